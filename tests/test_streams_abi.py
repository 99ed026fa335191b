"""The C ABI of many streams to finished frames (include/vss_streams.h): declared,
reachable through include/vss.h, exported by the library and bound in ctypes.
No GPU needed."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRY_POINTS = ["vss_background_composite_streams_device", "vss_segment_background_streams",
                "vss_video_process_streams", "vss_video_process_streams_device"]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vss_streams.h")).read(), flags=re.S)


def test_streams_abi_is_declared_exported_and_bound(pkg):
    assert '#include "vss_streams.h"' in open(os.path.join(ROOT, "include", "vss.h")).read()
    names = sorted(set(re.findall(r"\b(vss_[a-z0-9_]+)\s*\(", _header())))
    assert names == ENTRY_POINTS
    L = pkg.lib()
    for name in names:
        assert getattr(L, name).argtypes is not None, f"{name} has no ctypes signature in lib()"


def test_streams_signatures_match_the_header(pkg):
    """One ctypes argument per declared parameter."""
    src = _header()
    L = pkg.lib()
    for name in ENTRY_POINTS:
        params = re.search(r"\b" + name + r"\s*\(([^)]*)\)", src).group(1)
        assert len(getattr(L, name).argtypes) == len(params.split(",")), name


def test_python_methods_are_exported(pkg):
    assert callable(pkg.PostPool.replace_backgrounds)
    assert callable(pkg.composite_streams_device)
    assert callable(pkg.Video.process_streams)
    assert callable(pkg.Video.process_streams_device)


def test_null_objects_are_refused_without_a_gpu(pkg):
    """A null handle, video or pool: VSS_E_INVALID_ARG and a message, before any HIP call."""
    L = pkg.lib()
    buf = (ctypes.c_uint8 * 64)()
    ids = (ctypes.c_int * 1)(0)
    bgs = (ctypes.c_void_p * 1)(None)
    p = ctypes.addressof(buf)
    calls = [
        lambda: L.vss_background_composite_streams_device(None, bgs, 1, p, 2, 2, 4, 8, 16, p, p, 8, 16, None),
        lambda: L.vss_segment_background_streams(None, None, ids, bgs, p, 1, 2, 2, 4, 8, p),
        lambda: L.vss_video_process_streams_device(None, None, ids, bgs, None, p, 2, 4, p, 2, 2, 1, 2, 2, p, 2, 4, p,
                                                   2, 2, None),
        lambda: L.vss_video_process_streams(None, None, ids, bgs, p, p, 1, 2, 2, p, p),
    ]
    for call in calls:
        assert call() == pkg.VSS_E_INVALID_ARG
        assert L.vss_last_error(None)
