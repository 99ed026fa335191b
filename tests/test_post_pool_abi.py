"""The C ABI of the post chain over many streams (include/vss_pool.h): declared,
reachable through include/vss.h, exported by the library and bound in ctypes.
No GPU needed."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRY_POINTS = ["vss_post_pool_create", "vss_post_pool_destroy", "vss_post_pool_process_device",
                "vss_post_pool_reset", "vss_post_pool_set_config", "vss_segment_post_pool"]


def test_post_pool_abi_is_declared_exported_and_bound(pkg):
    assert '#include "vss_pool.h"' in open(os.path.join(ROOT, "include", "vss.h")).read()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vss_pool.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(vss_[a-z_]+)\s*\(", src)))
    assert names == ENTRY_POINTS
    L = pkg.lib()
    for name in names:
        assert getattr(L, name).argtypes is not None, f"{name} has no ctypes signature in lib()"


def test_post_pool_signatures_match_the_header(pkg):
    """One ctypes argument per declared parameter."""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vss_pool.h")).read(), flags=re.S)
    L = pkg.lib()
    for name in ENTRY_POINTS:
        params = re.search(r"\b" + name + r"\s*\(([^)]*)\)", src).group(1)
        assert len(getattr(L, name).argtypes) == len(params.split(",")), name


def test_python_class_is_exported(pkg):
    for m in ("process_device", "segment", "reset", "set_config", "close", "__enter__", "__exit__"):
        assert callable(getattr(pkg.PostPool, m))
