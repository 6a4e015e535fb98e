"""The distance-field entry points of the C ABI (f110qp_grid_distance_dev, f110qp_grid_inflate_dev,
f110qp_grid_lookup_dev, f110qp_grid_field, f110qp_wall_distance) without a GPU: exported symbols, every argument rule
(each answers before the first device call: on a machine without a device anything later would be F110QP_ERR_HIP)
with its word in last_error and nothing written, and the bindings' own checks."""
import ctypes as C
import os

import numpy as np
import pytest
from test_capi_world import NOT_FINITE, ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELD = ("f110qp_grid_distance_dev", "f110qp_grid_inflate_dev", "f110qp_grid_lookup_dev", "f110qp_grid_field",
         "f110qp_wall_distance")


def test_symbols_and_version(capi):
    hdr = open(os.path.join(ROOT, "include", "f110qp.h")).read()
    for name in FIELD:
        assert name + "(" in hdr and name in capi.EXPORTED
        assert getattr(capi.load(), name) is not None
        assert getattr(capi.load(test=True), name) is not None
    assert capi.load().f110qp_version() == 6 and "#define F110QP_API_VERSION 6" in hdr  # additive
    assert f"#define F110QP_FIELD_MAX_SIDE {capi.FIELD_MAX_SIDE}\n" in hdr
    for rule in ("D1. ", "D2. ", "D3. ", "D4. "):
        assert rule in hdr, rule


def invalid(capi, rc, word):
    assert rc == capi.ERR_INVALID, rc
    assert word in capi.last_error(), capi.last_error()


def cfg(capi, **over):
    return capi.default_grid_config(**{**dict(width=8, height=6, origin_x=-1.0, origin_y=0.5, resolution=0.1), **over})


def grid_rules(capi, call):
    """The grid family's rules on the config, then the field's limit on the sides."""
    invalid(capi, call(gc=None), "grid config")
    invalid(capi, call(gc=cfg(capi, width=-1)), "width")
    invalid(capi, call(gc=cfg(capi, height=-1)), "height")
    for v in NOT_FINITE + [0.0, -0.1]:
        invalid(capi, call(gc=cfg(capi, resolution=v)), "resolution")
    for v in NOT_FINITE + [-0.1]:
        invalid(capi, call(gc=cfg(capi, reach=v)), "reach")
    for k in ("origin_x", "origin_y"):
        for v in NOT_FINITE:
            invalid(capi, call(gc=cfg(capi, **{k: v})), "origin")
    for w, h in ((32769, 1), (1, 32769), (32769, 32769), (1 << 20, 1)):
        invalid(capi, call(gc=cfg(capi, width=w, height=h)), "width and height must be <= 32768")
    invalid(capi, call(gc=cfg(capi, width=1 << 16, height=1 << 16)), "width * height")  # the family's own rule first


@pytest.fixture
def host():
    buf = np.zeros(1 << 16, np.float64)
    return buf, C.c_void_p(buf.ctypes.data)


def test_distance_validation_errors_touch_no_device(capi, host):
    buf, p = host

    def call(gc=cfg(capi), grid=p, d2=p, nearest=p, work=p):
        return capi.load().f110qp_grid_distance_dev(ref(gc), grid, d2, nearest, work, None)

    grid_rules(capi, call)
    invalid(capi, call(grid=None), "needs the grid")
    for k in ("d2", "work"):
        invalid(capi, call(**{k: None}), "non-NULL")
    for w, h in ((0, 0), (0, 6), (8, 0)):  # no cell: nothing to do, whatever the pointers
        assert call(gc=cfg(capi, width=w, height=h), grid=None, d2=None, nearest=None, work=None) == capi.OK
    assert not buf.any(), "nothing was written"


def test_inflate_validation_errors_touch_no_device(capi, host):
    buf, p = host

    def call(gc=cfg(capi), d2=p, radius=0.3, out=p):
        return capi.load().f110qp_grid_inflate_dev(ref(gc), d2, radius, out, None)

    grid_rules(capi, call)
    for v in NOT_FINITE + [-0.001, -1.0]:
        invalid(capi, call(radius=v), "radius")
        invalid(capi, call(radius=v, gc=cfg(capi, width=0)), "radius")
    for k in ("d2", "out"):
        invalid(capi, call(**{k: None}), "non-NULL")
    assert call(gc=cfg(capi, width=0), d2=None, out=None) == capi.OK
    assert not buf.any(), "nothing was written"


def lookup_rules(capi, call):
    for v in (0, -1):
        invalid(capi, call(batch=v), "batch")
        invalid(capi, call(rows=v), "rows")
    invalid(capi, call(batch=1 << 16, rows=(1 << 14) + 1), "too large")
    for k in ("x", "dist"):
        invalid(capi, call(**{k: None}), "non-NULL")


def test_lookup_validation_errors_touch_no_device(capi, host):
    buf, p = host

    def call(gc=cfg(capi), d2=p, nearest=p, batch=8, rows=3, x=p, dist=p, cell=p):
        return capi.load().f110qp_grid_lookup_dev(ref(gc), d2, nearest, batch, rows, x, dist, cell, None)

    grid_rules(capi, call)
    lookup_rules(capi, call)
    invalid(capi, call(nearest=None), "nearest and cell")
    invalid(capi, call(cell=None), "nearest and cell")
    invalid(capi, call(d2=None), "needs d2")
    assert not buf.any(), "nothing was written"


def test_host_calls_validation_errors_touch_no_device(capi, host):
    buf, p = host

    def field(gc=cfg(capi), grid=p, radius=0.3, d2=p, nearest=p, inflated=p):
        return capi.load().f110qp_grid_field(ref(gc), grid, radius, d2, nearest, inflated)

    grid_rules(capi, field)
    invalid(capi, field(grid=None), "needs the grid")
    invalid(capi, field(d2=None), "non-NULL")
    for v in NOT_FINITE + [-0.5]:
        invalid(capi, field(radius=v), "radius")
    assert field(gc=cfg(capi, height=0), grid=None, d2=None, nearest=None, inflated=None) == capi.OK

    def wall(gc=cfg(capi), grid=p, batch=8, rows=3, x=p, dist=p, cell=p):
        return capi.load().f110qp_wall_distance(ref(gc), grid, batch, rows, x, dist, cell)

    grid_rules(capi, wall)
    lookup_rules(capi, wall)
    invalid(capi, wall(grid=None), "needs the grid")
    assert not buf.any(), "nothing was written"


def test_binding_checks_types_and_shapes(capi):
    torch = pytest.importorskip("torch")
    gc = cfg(capi)  # 8 x 6 = 48 cells
    u8, i32 = torch.zeros(64, dtype=torch.uint8), torch.zeros(64, dtype=torch.int32)
    f64, f32 = torch.zeros(256, dtype=torch.float64), torch.zeros(256, dtype=torch.float32)
    with pytest.raises(capi.F110QPError, match="grid_cfg must be a GridConfig"):
        capi.grid_distance_dev(None, u8, i32, i32)
    with pytest.raises(capi.F110QPError, match="width and height must be in 0..32768"):
        capi.grid_distance_dev(cfg(capi, width=32769), u8, i32, i32)
    with pytest.raises(capi.F110QPError, match="grid must be torch.uint8"):
        capi.grid_distance_dev(gc, i32, i32, i32)
    with pytest.raises(capi.F110QPError, match="grid holds 47 elements, the call needs 48"):
        capi.grid_distance_dev(gc, u8[:47], i32, i32)
    with pytest.raises(capi.F110QPError, match="d2 must be torch.int32"):
        capi.grid_distance_dev(gc, u8, f32, i32)
    with pytest.raises(capi.F110QPError, match="work holds"):
        capi.grid_distance_dev(gc, u8, i32, i32[:40])
    with pytest.raises(capi.F110QPError, match="work is required"):
        capi.grid_distance_dev(gc, u8, i32, None)
    with pytest.raises(capi.F110QPError, match="nearest must be torch.int32"):
        capi.grid_distance_dev(gc, u8, i32, i32, nearest=f64)
    with pytest.raises(capi.F110QPError, match="device"):
        capi.grid_distance_dev(gc, u8, i32, i32)  # host tensors
    with pytest.raises(capi.F110QPError, match="out must be torch.uint8"):
        capi.grid_inflate_dev(gc, i32, 0.3, i32)
    with pytest.raises(capi.F110QPError, match="d2 holds"):
        capi.grid_inflate_dev(gc, i32[:47], 0.3, u8)
    x = f64[:72].view(3, 8, 3)
    with pytest.raises(capi.F110QPError, match=r"x must be \[rows, B, 3\]"):
        capi.grid_lookup_dev(gc, i32, f64[:48].view(3, 8, 2), f64)
    with pytest.raises(capi.F110QPError, match="x must be torch.float64"):
        capi.grid_lookup_dev(gc, i32, f32[:72].view(3, 8, 3), f64)
    with pytest.raises(capi.F110QPError, match="given together"):
        capi.grid_lookup_dev(gc, i32, x, f64, nearest=i32)
    with pytest.raises(capi.F110QPError, match="given together"):
        capi.grid_lookup_dev(gc, i32, x, f64, cell=i32)
    with pytest.raises(capi.F110QPError, match="dist holds 23 elements, the call needs 24"):
        capi.grid_lookup_dev(gc, i32, x, f64[:23])
    with pytest.raises(capi.F110QPError, match="cell must be torch.int32"):
        capi.grid_lookup_dev(gc, i32, x, f64, nearest=i32, cell=f64)
    with pytest.raises(capi.F110QPError, match="nearest holds"):
        capi.grid_lookup_dev(gc, i32, x, f64, nearest=i32[:47], cell=i32)
    g = np.zeros((6, 8), np.uint8)
    with pytest.raises(capi.F110QPError, match="grid must be a uint8 numpy array"):
        capi.grid_field(gc, g.astype(np.int32))
    with pytest.raises(capi.F110QPError, match=r"\[6, 8\]"):
        capi.grid_field(gc, g.T.copy())
    with pytest.raises(capi.F110QPError, match="float64"):
        capi.wall_distance(gc, g, np.zeros((3, 8, 3), np.float32))
    with pytest.raises(capi.F110QPError, match=r"x must be \[rows, B, 3\]"):
        capi.wall_distance(gc, g, np.zeros((3, 8, 2)))
