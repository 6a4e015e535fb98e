"""The noisy-LiDAR entry points of the C ABI (f110qp_default_noise_config, f110qp_cast_scans_noisy_dev,
f110qp_rollout_noisy[_dev]) without a GPU: exported symbols, the default, the struct layout against the header, and
every argument rule, each of which answers before the first device call."""
import ctypes as C
import os
import re

import numpy as np
import pytest
from test_capi_walls import wall_rules
from test_capi_world import ref, scan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOISY = ("f110qp_default_noise_config", "f110qp_cast_scans_noisy_dev", "f110qp_rollout_noisy_dev",
         "f110qp_rollout_noisy")
LLONG_MAX = 2 ** 63 - 1


def test_symbols_and_version(capi):
    hdr = open(os.path.join(ROOT, "include", "f110qp.h")).read()
    for name in NOISY:
        assert name + "(" in hdr and name in capi.EXPORTED
        assert getattr(capi.load(), name) is not None
        assert getattr(capi.load(test=True), name) is not None
    assert capi.load().f110qp_version() == 6 and "#define F110QP_API_VERSION 6" in hdr  # additive


def test_default_and_layout(capi):
    nz = capi.NoiseConfig(seed=9, car_base=9, sigma_abs=9.0, sigma_rel=9.0, dropout=0.9)
    capi.load().f110qp_default_noise_config(C.byref(nz))
    assert (nz.seed, nz.car_base, nz.sigma_abs, nz.sigma_rel, nz.dropout) == (0, 0, 0.0, 0.0, 0.0)
    assert bytes(nz) == bytes(C.sizeof(nz)), "the default is all zero"
    d = capi.default_noise_config()
    assert bytes(d) == bytes(C.sizeof(d))
    k = capi.default_noise_config(seed=2 ** 63 + 5, car_base=2 ** 40, sigma_abs=0.01, sigma_rel=0.02, dropout=0.5)
    assert (k.seed, k.car_base, k.sigma_abs, k.sigma_rel, k.dropout) == (2 ** 63 + 5, 2 ** 40, 0.01, 0.02, 0.5)
    capi.load().f110qp_default_noise_config(None)  # a NULL config is ignored
    hdr = open(os.path.join(ROOT, "include", "f110qp.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} f110qp_noise_config;", hdr).group(1)
    fields = re.findall(r"^\s*(unsigned long long|long long|int|double|float)\s+(\w+);", body, re.M)
    ctype = {"unsigned long long": C.c_ulonglong, "long long": C.c_longlong, "int": C.c_int, "double": C.c_double,
             "float": C.c_float}
    assert [(n, ctype[t]) for t, n in fields] == list(capi.NoiseConfig._fields_)
    assert C.sizeof(capi.NoiseConfig) == 40


def noise_rules(capi, call, B):
    """The noise rules shared by the three calls; call(noise=...) -> return code."""
    ok = dict(seed=1, car_base=0, sigma_abs=0.01, sigma_rel=0.01, dropout=0.1)

    def cfg(**over):
        return capi.default_noise_config(**{**ok, **over})

    assert call(noise=None) == capi.ERR_INVALID and "noise config" in capi.last_error()
    for k in ("sigma_abs", "sigma_rel"):
        for v in (-1e-300, -1.0, float("inf"), -float("inf"), float("nan")):
            assert call(noise=cfg(**{k: v})) == capi.ERR_INVALID, (k, v)
            assert "sigma" in capi.last_error()
    for v in (-1e-300, 1.0000000000000002, 2.0, float("inf"), float("nan")):
        assert call(noise=cfg(dropout=v)) == capi.ERR_INVALID, v
        assert "dropout" in capi.last_error()
    for v in (-1, -(2 ** 63)):
        assert call(noise=cfg(car_base=v)) == capi.ERR_INVALID, v
        assert "car_base" in capi.last_error()
    for v in (LLONG_MAX, LLONG_MAX - B + 1):
        assert call(noise=cfg(car_base=v)) == capi.ERR_INVALID, v
        assert "car_base + batch" in capi.last_error()


def test_cast_validation_errors_touch_no_device(capi):
    L = capi.load()
    buf = np.zeros(4096, np.float64)
    p = C.c_void_p(buf.ctypes.data)
    sc, wc = scan(capi), capi.default_world_config(num_circles=5)
    race, body = capi.default_race_config(group_size=2), capi.default_body_config()
    ok, quiet = capi.default_walls_config(num_segments=3), capi.default_noise_config()

    def cast(walls=ok, segments=p, batch=4, body=body, race=race, wc=wc, circles=p, noise=quiet, tick=0, sc=sc,
             lst=None, count=None):
        return L.f110qp_cast_scans_noisy_dev(ref(sc), ref(wc), ref(race), ref(body), ref(walls), ref(noise), batch, tick,
                                             lst, count, p, circles, segments, p, None)

    noise_rules(capi, cast, 4)
    for t in (-1, -(2 ** 31)):
        assert cast(tick=t) == capi.ERR_INVALID and "tick" in capi.last_error()
    # every rule of the walls cast still answers
    wall_rules(capi, cast, 4)
    assert cast(sc=None) == capi.ERR_INVALID and "scan config" in capi.last_error()
    assert cast(body=None) == capi.ERR_INVALID and "body config" in capi.last_error()
    assert cast(race=None) == capi.ERR_INVALID and "race config" in capi.last_error()
    assert cast(wc=None) == capi.ERR_INVALID and "world config" in capi.last_error()
    assert cast(batch=3) == capi.ERR_INVALID and "group_size" in capi.last_error()
    assert cast(batch=-1) == capi.ERR_INVALID and "batch" in capi.last_error()
    assert cast(lst=p) == capi.ERR_INVALID and "together" in capi.last_error()
    # the noise is checked where the batch is empty; the walls' rules come first
    assert cast(batch=0, noise=None) == capi.ERR_INVALID and "noise config" in capi.last_error()
    assert cast(walls=None, noise=None) == capi.ERR_INVALID and "walls config" in capi.last_error()
    assert cast(batch=0) == capi.OK
    assert cast(batch=0, tick=2 ** 31 - 1, noise=capi.default_noise_config(car_base=LLONG_MAX, dropout=1.0)) == capi.OK
    assert cast(batch=0, walls=capi.default_walls_config(), segments=None) == capi.OK


@pytest.mark.parametrize("name", ["f110qp_rollout_noisy_dev", "f110qp_rollout_noisy"])
def test_rollout_noisy_validation_errors_touch_no_device(capi, name):
    fn = getattr(capi.load(), name)
    dev = name.endswith("_dev")
    s = capi.Solver(capi.default_config(20, x_ref_points=50))
    buf = np.zeros(4096, np.float64)
    p = C.c_void_p(buf.ctypes.data)
    rc, rp = capi.default_rollout_config(ticks=3), capi.default_replan_config(num_waypoints=4)
    sc, wc = scan(capi), capi.default_world_config(num_circles=5)
    race, cc, body = capi.default_race_config(group_size=2), capi.default_contact_config(), capi.default_body_config()
    ok, every, quiet = capi.default_walls_config(num_segments=3), capi.default_refresh_config(every=1), \
        capi.default_noise_config()

    def call(walls=ok, segments=p, batch=4, body=body, cc=cc, rf=every, noise=quiet, patch=None):
        # 0 table, 1 waypoints, 2 x_ref, 3 have_path, 4 circles, 5 segments, 6 x_traj, 7 u_lin_traj, 8 u_applied,
        # 9 status_traj, then the optional iters .. ranges_traj (11), clear_traj, nearest_traj, crash_tick[, stream]
        a = [p] * 5 + [segments] + [p] * 4 + [None] * 11 + [p, None, p] + ([None] if dev else [])
        for k, v in (patch or {}).items():
            a[k] = v
        return fn(s._h, ref(rc), ref(sc), ref(rp), ref(wc), ref(race), ref(cc), ref(body), ref(walls), ref(rf),
                  ref(noise), batch, *a)

    noise_rules(capi, call, 4)
    # the noise is checked where the batch is empty
    assert call(noise=None, batch=0) == capi.ERR_INVALID and "noise config" in capi.last_error()
    # every check of the refresh call
    assert call(rf=None) == capi.ERR_INVALID and "refresh config" in capi.last_error()
    assert call(rf=capi.default_refresh_config(every=-1)) == capi.ERR_INVALID and "every" in capi.last_error()
    wall_rules(capi, call, 4)
    assert call(body=None) == capi.ERR_INVALID and "body config" in capi.last_error()
    assert call(cc=None) == capi.ERR_INVALID and "contact config" in capi.last_error()
    assert call(patch={21: None}) == capi.ERR_INVALID and "clear_traj" in capi.last_error()
    assert call(patch={23: None}) == capi.ERR_INVALID and "crash_tick" in capi.last_error()
    assert call(patch={6: None}) == capi.ERR_INVALID and "x_traj" in capi.last_error()
    assert call(batch=0) == capi.OK
    assert call(batch=0, noise=capi.default_noise_config(seed=2 ** 64 - 1, sigma_abs=1.0, dropout=1.0)) == capi.OK
    s.close()


def test_binding_checks(capi):
    s = capi.Solver(capi.default_config(20, x_ref_points=50))
    cfg = (capi.default_race_config(), capi.default_contact_config(), capi.default_body_config())
    with pytest.raises(capi.F110QPError, match="NoiseConfig"):
        s.rollout_noisy(None, None, None, None, *cfg, capi.default_refresh_config(), None, None, None, None, None, 1)
    with pytest.raises(capi.F110QPError, match="NoiseConfig"):
        s.rollout_noisy_dev(None, None, None, None, *cfg, capi.default_walls_config(), capi.default_refresh_config(), 3,
                            *[None] * 12)
    s.close()
