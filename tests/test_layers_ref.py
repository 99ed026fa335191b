"""The definition of the branding layers (include/vss_layers.h) on its numpy
restatement (tests/layers_ref.py), the host-only parts of the library
(vss_layers_map, the exported symbols) and the template helper.  No GPU needed."""
import json
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import layers_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANVAS = (1920, 1080)
ENTRY_POINTS = ["vss_background_overlay_device", "vss_background_set_layers", "vss_background_set_privacy",
                "vss_layers_map"]


def _rect(x, y, w, h, color, radius=0, privacy=1, shadow=None):
    return {"type": "rect", "privacy": privacy, "x": x, "y": y, "width": w, "height": h, "color": color,
            "radius": radius, "shadow": shadow}


def _sprite(seed, h, w):
    px = np.random.default_rng(seed).integers(0, 256, (h, w, 4), dtype=np.uint8)
    px[: h // 3, :, 3] = 0
    px[-(h // 3):, :, 3] = 255
    return px


@pytest.fixture(scope="module")
def scene(oracle, pkg):
    """A plate with every kind of layer on a 45 x 150 frame; built once."""
    layers = [
        _rect(100, 100, 900, 500, (10, 200, 90, 128), radius=120),
        {"type": "image", "privacy": 1, "x": 600, "y": 300, "width": 700, "height": 600, "pixels": _sprite(1, 9, 11),
         "shadow": {"color": (0, 0, 0, 180), "blur": 60, "dx": 40, "dy": 30}},
        _rect(-200, 700, 1500, 600, (255, 255, 255, 200), radius=40, privacy=2,
              shadow={"color": (20, 30, 40, 255), "blur": 0, "dx": -30, "dy": -30}),
        _rect(1500, 50, 300, 300, (1, 2, 3, 255), privacy=3),
    ]
    return layers, {lv: ref.overlay(oracle, pkg, layers, lv, CANVAS, 45, 150) for lv in (1, 2, 3)}


def test_plate_is_premultiplied(scene):
    for O in scene[1].values():
        assert O.any()
        assert np.all(O[..., :3] <= O[..., 3:4])


def test_no_visible_layer_is_the_identity(oracle, pkg, scene):
    layers = [dict(l, privacy=3) for l in scene[0]]
    O = ref.overlay(oracle, pkg, layers, 2, CANVAS, 45, 150)
    assert not O.any()
    bg = np.random.default_rng(0).integers(0, 256, (45, 150, 3), dtype=np.uint8)
    assert np.array_equal(ref.under(bg, O), bg)
    assert not ref.overlay(oracle, pkg, [], 3, CANVAS, 45, 150).any()


def test_privacy_levels_nest(scene):
    """The opaque level-3 rectangle shows at level 3 only; level 1 lacks the level-2 plate."""
    O = scene[1]
    y, x = ref.lmap(200, 1080, 45), ref.lmap(1650, 1920, 150)
    assert tuple(O[3][y, x]) == (1, 2, 3, 255) and tuple(O[2][y, x]) == (0, 0, 0, 0)
    assert not np.array_equal(O[1], O[2])


@pytest.mark.parametrize("geom", [(3, 5, 40, 29, 9), (0, 0, 17, 17, 8), (2, 2, 30, 12, 5), (1, 1, 9, 20, 1)])
def test_rounded_rect_coverage_is_symmetric(geom):
    X0, Y0, X1, Y1, R = geom  # R within half of either side, as the clamp leaves it
    n = ref.rect_coverage(X0, Y0, X1, Y1, R, range(X0, X1), range(Y0, Y1))
    assert np.array_equal(n, n[::-1]) and np.array_equal(n, n[:, ::-1])
    assert n.max() == 16 and n.min() < 16  # the corners are cut
    assert np.all(n[R:-R, :] == 16) and np.all(n[:, R:-R] == 16)


def test_radius_zero_is_a_plain_rectangle(oracle, pkg):
    n = ref.rect_coverage(4, 3, 20, 11, 0, range(0, 30), range(0, 20))
    want = np.zeros((20, 30), np.int64)
    want[3:11, 4:20] = 16
    assert np.array_equal(n, want)
    O = ref.overlay(oracle, pkg, [_rect(4, 3, 16, 8, (200, 100, 50, 255))], 1, (30, 20), 20, 30)
    assert np.all(O[3:11, 4:20] == (200, 100, 50, 255))
    O[3:11, 4:20] = 0
    assert not O.any()


def test_capsule_when_the_radius_exceeds_half_the_side():
    """R clamps to half the shorter side: the ends are half discs."""
    assert min(ref.lmap(500, 100, 100), (40 - 0) // 2, (10 - 0) // 2) == 5
    n = ref.rect_coverage(0, 0, 40, 10, 5, range(40), range(10))
    assert n[0, 0] < 16 and n[9, 39] < 16 and np.all(n[:, 5:35] == 16) and n[4, 0] == 16


def test_an_opaque_layer_replaces_what_is_under_it(oracle, pkg):
    under = _rect(0, 0, 30, 20, (9, 99, 199, 140))
    top = _rect(5, 5, 10, 10, (70, 80, 90, 255))
    O = ref.overlay(oracle, pkg, [under, top], 1, (30, 20), 20, 30)
    assert np.all(O[5:15, 5:15] == (70, 80, 90, 255))
    bg = np.full((20, 30, 3), 255, np.uint8)
    assert np.all(ref.under(bg, O)[5:15, 5:15] == (70, 80, 90))


def test_order_matters_for_translucent_layers(oracle, pkg):
    a = _rect(0, 0, 20, 20, (255, 0, 0, 128))
    b = _rect(10, 0, 20, 20, (0, 0, 255, 128))
    ab = ref.overlay(oracle, pkg, [a, b], 1, (30, 20), 20, 30)
    ba = ref.overlay(oracle, pkg, [b, a], 1, (30, 20), 20, 30)
    assert not np.array_equal(ab[:, 10:20], ba[:, 10:20])
    assert np.array_equal(ab[:, :10], ba[:, :10]) and np.array_equal(ab[:, 20:], ba[:, 20:])
    assert np.array_equal(ab[..., 3], ba[..., 3])  # the alpha does not depend on the order


def test_abutting_layers_abut_on_the_frame():
    for fw in (53, 150, 1280, 2560):
        for x in range(-50, 2000, 37):
            assert ref.lmap(x + 113, 1920, fw) - ref.lmap(x, 1920, fw) >= 0
    assert ref.lmap(-1, 2, 1) == 0 and ref.lmap(-3, 2, 1) == -1 and ref.lmap(1, 2, 1) == 1  # half rounds up


def test_layers_map_matches_the_definition(pkg):
    for canvas, frame in [(1920, 150), (1080, 45), (1920, 1920), (7, 53), (1920, 3840), (3, 1000), (1, 1)]:
        for v in list(range(-300, 300, 7)) + [-100000, -1921, -1, 0, 1, 959, 960, 961, 1919, 1920, 5000, 1 << 20]:
            assert pkg.layers_map(v, canvas, frame) == ref.lmap(v, canvas, frame), (v, canvas, frame)


def test_layers_abi_is_declared_exported_and_bound(pkg):
    assert '#include "vss_layers.h"' in open(os.path.join(ROOT, "include", "vss.h")).read()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vss_layers.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(vss_[a-z_]+)\s*\(", src)))
    assert names == ENTRY_POINTS
    L = pkg.lib()
    for name in names:
        params = re.search(r"\b" + name + r"\s*\(([^)]*)\)", src).group(1)
        assert len(getattr(L, name).argtypes) == len(params.split(",")), name
    for m in ("set_layers", "set_privacy", "overlay"):
        assert callable(getattr(pkg.Background, m))


# ---- template_layers on the reference's templates ---------------------------------
FIELDS = {"full_name": "A B", "position": "Engineer", "department": "R&D", "company": "ACME", "office_location": "HQ",
          "email": "a@b.c", "telegram": "@ab", "slogan": "Hello"}


def _rasterize(text, font, color):
    """A solid block: 10 px per character wide, 20 high, the baseline 15 below the top."""
    px = np.zeros((20, 10 * len(text), 4), np.uint8)
    px[:] = color
    return px, 15


@pytest.fixture(scope="module")
def templates():
    with open(os.path.join(ROOT, "tests", "golden", "branding_templates.json"), encoding="utf-8") as f:
        data = json.load(f)
    assert list(data) == ["templates"]
    return data["templates"]


def _images():
    return {k: np.full((8, 8, 4), 255, np.uint8) for k in ("email_icon", "telegram_icon", "qr_code", "company_logo")}


@pytest.mark.parametrize("name,count,by_privacy", [("corporate_violet", 12, (2, 5, 5)),
                                                   ("corporate__rect", 15, (3, 6, 6))])
def test_template_layers_counts(pkg, templates, name, count, by_privacy):
    layers = pkg.template_layers(templates[name], FIELDS, _images(), _rasterize)
    assert len(layers) == count
    assert tuple(sum(1 for l in layers if l.privacy == p) for p in (1, 2, 3)) == by_privacy


def test_template_layers_follow_update_canvas(pkg, templates):
    t = templates["corporate__rect"]
    layers = pkg.template_layers(t, FIELDS, _images(), _rasterize)
    logo_t = next(l for l in t["layers"] if l.get("content") == "company_logo")
    assert "shadow" in logo_t  # the template carries one, updateCanvas ignores it (:53)
    logo = next(l for l in layers if l.type == "image" and (l.x, l.y) == (logo_t["x"], logo_t["y"]))
    assert logo.shadow is None and (logo.width, logo.height) == (logo_t["width"], logo_t["height"])
    email_t = next(l for l in t["layers"] if l.get("content") == "email")
    w = 10 * len(FIELDS["email"])
    email = next(l for l in layers if l.width == w and l.y == email_t["y"] - 15)
    assert email_t["align"] == "right" and email.x == email_t["x"] - w
    assert email.shadow == {"color": (0, 0, 0, 179), "blur": 5, "dx": 2, "dy": 2}  # rgba(0,0,0,0.7)
    dept_t = next(l for l in t["layers"] if l.get("content") == "department_and_company")
    lines = [l for l in layers if l.x == dept_t["x"] and l.y in (dept_t["y"] - 15, dept_t["y"] + 40 - 15)]
    assert [l.width for l in lines] == [10 * len("R&D"), 10 * len("ACME")]
    rect = layers[0]
    assert rect.type == "rect" and rect.color == (0, 0, 0, 64) and rect.radius == 20  # rgba(0, 0, 0, 0.25)
    assert tuple(layers[3].pixels[0, 0]) == (255, 255, 255, 255)  # '#FFFFFF' reached the rasteriser
    # an image whose key is absent is skipped (:69)
    fewer = pkg.template_layers(t, FIELDS, {}, _rasterize)
    assert len(fewer) == 15 - 4
    # multi-line text: one layer per line at y + i*lineHeight
    multi = pkg.template_layers(t, dict(FIELDS, office_location="HQ\nFloor 3"), _images(), _rasterize)
    assert len(multi) == 16


def test_parse_color(pkg):
    assert pkg.parse_color("#E0E0E0") == (224, 224, 224, 255)
    assert pkg.parse_color("rgba(0, 0, 0, 0.25)") == (0, 0, 0, 64)
    assert pkg.parse_color("rgba(0,0,0,0.5)") == (0, 0, 0, 128)
    assert pkg.parse_color("rgba(1,2,3,1)") == (1, 2, 3, 255)
