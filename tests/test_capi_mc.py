"""The Monte Carlo entry points of the C ABI (f110qp_default_mc_config, f110qp_mc_fan_dev, f110qp_mc_survival_dev,
f110qp_mc_outcomes_dev, f110qp_mc_summary) without a GPU: exported symbols, every argument rule (each answers
before the first device call: on a machine without a device anything later would be F110QP_ERR_HIP) with its word
in last_error and nothing written, and the bindings' own checks."""
import ctypes as C
import os

import numpy as np
import pytest
from test_capi_world import NOT_FINITE, ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MC = ("f110qp_default_mc_config", "f110qp_mc_fan_dev", "f110qp_mc_survival_dev", "f110qp_mc_outcomes_dev",
      "f110qp_mc_summary")


def test_symbols_and_version(capi):
    hdr = open(os.path.join(ROOT, "include", "f110qp.h")).read()
    for name in MC:
        assert name + "(" in hdr and name in capi.EXPORTED
        assert getattr(capi.load(), name) is not None
        assert getattr(capi.load(test=True), name) is not None
    assert capi.load().f110qp_version() == 6 and "#define F110QP_API_VERSION 6" in hdr  # additive
    assert f"#define F110QP_MC_MAX_HYPOTHESES {capi.MC_MAX_HYPOTHESES}\n" in hdr
    assert f"#define F110QP_MC_MAX_PROBS {capi.MC_MAX_PROBS}\n" in hdr


def test_default_config(capi):
    for lib in (False, True):
        c = capi.McConfig(7, 7, 7, (7.0,) * 8)
        capi.load(test=lib).f110qp_default_mc_config(C.byref(c))
        assert (c.hypotheses, c.group_size, c.num_probs) == (1, 1, 3) and list(c.prob) == [0.0, 0.5, 1.0] + [0.0] * 5
    capi.load().f110qp_default_mc_config(None)  # ignored
    c = capi.default_mc_config(hypotheses=16, group_size=2, prob=(0.1, 0.9))
    assert (c.hypotheses, c.group_size, c.num_probs) == (16, 2, 2) and list(c.prob)[:3] == [0.1, 0.9, 0.0]
    assert capi.default_mc_config(prob=(0.1, 0.9), num_probs=1).num_probs == 1
    with pytest.raises(capi.F110QPError, match="at most 8"):
        capi.default_mc_config(prob=[0.5] * 9)
    assert C.sizeof(capi.McConfig) == 16 + 8 * 8


def invalid(capi, rc, word):
    assert rc == capi.ERR_INVALID, rc
    assert word in capi.last_error(), capi.last_error()


def config_rules(capi, call, B):
    """The rules on the config, for a call whose valid default is M x G = B / 2."""
    invalid(capi, call(mc=None), "mc config")
    for M in (0, -1, 4097, 1 << 20):
        invalid(capi, call(mc=capi.default_mc_config(hypotheses=M)), "hypotheses")
    for G in (0, -1, -B):
        invalid(capi, call(mc=capi.default_mc_config(group_size=G)), "group_size")
    for v in (0, -1, -B):
        invalid(capi, call(batch=v), "batch")
    for M, G in ((B - 1, 1), (1, B + 1), (B, 2), (3, 1), (2, 1 << 30), (4096, 1 << 20)):
        invalid(capi, call(mc=capi.default_mc_config(hypotheses=M, group_size=G)), "multiple of hypotheses x group_size")
    for Q in (0, -1, 9):
        invalid(capi, call(mc=capi.default_mc_config(num_probs=Q)), "num_probs")
    for v in NOT_FINITE + [-0.001, 1.001, -1.0]:
        invalid(capi, call(mc=capi.default_mc_config(prob=(0.5, v))), "prob")
        invalid(capi, call(mc=capi.default_mc_config(prob=(v,))), "prob")


@pytest.fixture
def host():
    buf = np.zeros(4096, np.float64)
    return buf, C.c_void_p(buf.ctypes.data)


def test_fan_validation_errors_touch_no_device(capi, host):
    buf, p = host
    mc_ok = capi.default_mc_config(hypotheses=2, group_size=2)

    def call(mc=mc_ok, batch=8, rows=3, v=p, fan=p, count=None):
        return capi.load().f110qp_mc_fan_dev(ref(mc), batch, rows, v, fan, count, None)

    config_rules(capi, call, 8)
    for v in (0, -1):
        invalid(capi, call(rows=v), "rows")
    invalid(capi, call(batch=1 << 16, rows=(1 << 14) + 1), "too large")
    for k in ("v", "fan"):
        invalid(capi, call(**{k: None}), "non-NULL")
    assert not buf.any(), "nothing was written"


def test_survival_validation_errors_touch_no_device(capi, host):
    buf, p = host
    mc_ok = capi.default_mc_config(hypotheses=2, group_size=2)

    def call(mc=mc_ok, batch=8, ticks=3, crash=p, alive=p, crashed=None):
        return capi.load().f110qp_mc_survival_dev(ref(mc), batch, ticks, crash, alive, crashed, None)

    config_rules(capi, call, 8)
    for v in (0, -1):
        invalid(capi, call(ticks=v), "ticks")
    invalid(capi, call(batch=1 << 16, ticks=1 << 14), "too large")  # rows = ticks + 1
    invalid(capi, call(batch=8, ticks=np.iinfo(np.int32).max), "too large")
    for k in ("crash", "alive"):
        invalid(capi, call(**{k: None}), "non-NULL")
    assert not buf.any(), "nothing was written"


def outcome_rules(capi, call):
    for v in (0, -1):
        invalid(capi, call(batch=v), "batch")
        invalid(capi, call(ticks=v), "ticks")
    invalid(capi, call(batch=1 << 16, ticks=1 << 14), "too large")
    for k in ("clear", "min_clear"):
        invalid(capi, call(**{k: None}), "non-NULL")
    invalid(capi, call(status=None), "status_traj")
    invalid(capi, call(status=None, first=None), "status_traj")
    invalid(capi, call(status=None, unsolved=None), "status_traj")
    invalid(capi, call(kind=None), "kind_traj")


def test_outcomes_validation_errors_touch_no_device(capi, host):
    buf, p = host

    def call(batch=8, ticks=3, clear=p, status=p, kind=p, min_clear=p, min_row=p, unsolved=p, first=p, pf=p):
        return capi.load().f110qp_mc_outcomes_dev(batch, ticks, clear, status, kind, min_clear, min_row, unsolved, first,
                                                  pf, None)

    outcome_rules(capi, call)
    assert not buf.any(), "nothing was written"


def test_summary_validation_errors_touch_no_device(capi, host):
    buf, p = host
    mc_ok = capi.default_mc_config(hypotheses=2, group_size=2)

    def call(mc=mc_ok, batch=8, ticks=3, clear=p, crash=p, status=p, kind=p, fan=p, count=None, alive=p, crashed=None,
             min_clear=p, min_row=p, unsolved=p, first=p, pf=p):
        return capi.load().f110qp_mc_summary(ref(mc), batch, ticks, clear, crash, status, kind, fan, count, alive, crashed,
                                             min_clear, min_row, unsolved, first, pf)

    config_rules(capi, call, 8)
    outcome_rules(capi, call)
    for k in ("crash", "fan", "alive"):
        invalid(capi, call(**{k: None}), "non-NULL")
    assert not buf.any(), "nothing was written"


def test_binding_checks_types_and_shapes(capi):
    torch = pytest.importorskip("torch")
    t32, t64 = torch.zeros(256, dtype=torch.float32), torch.zeros(256, dtype=torch.float64)
    i32 = torch.zeros(64, dtype=torch.int32)
    mc = capi.default_mc_config(hypotheses=2, group_size=2)
    v = t64[:24].view(3, 8)
    with pytest.raises(capi.F110QPError, match=r"v must be \[rows, B\]"):
        capi.mc_fan_dev(mc, t64[:24].view(3, 4, 2), t64, i32)
    with pytest.raises(capi.F110QPError, match="v must be torch.float64"):
        capi.mc_fan_dev(mc, t32[:24].view(3, 8), t64)
    with pytest.raises(capi.F110QPError, match="must divide B = 8, got 3 x 2"):
        capi.mc_fan_dev(capi.default_mc_config(hypotheses=3, group_size=2), v, t64)
    with pytest.raises(capi.F110QPError, match="hypotheses must be in"):
        capi.mc_fan_dev(capi.default_mc_config(hypotheses=0), v, t64)
    with pytest.raises(capi.F110QPError, match="num_probs must be in"):
        capi.mc_fan_dev(capi.default_mc_config(hypotheses=2, num_probs=9), v, t64)
    with pytest.raises(capi.F110QPError, match="fan holds 35 elements, the call needs 36"):
        capi.mc_fan_dev(mc, v, t64[:35])
    with pytest.raises(capi.F110QPError, match="count must be torch.int32"):
        capi.mc_fan_dev(mc, v, t64, t64)
    with pytest.raises(capi.F110QPError, match="count holds"):
        capi.mc_fan_dev(mc, v, t64, i32[:11])
    with pytest.raises(capi.F110QPError, match="crash_tick must be"):
        capi.mc_survival_dev(mc, i32[:8].view(2, 4), 3, i32)
    with pytest.raises(capi.F110QPError, match="crash_tick must be torch.int32"):
        capi.mc_survival_dev(mc, t64[:8], 3, i32)
    with pytest.raises(capi.F110QPError, match="ticks must be"):
        capi.mc_survival_dev(mc, i32[:8], 0, i32)
    with pytest.raises(capi.F110QPError, match="alive holds 15 elements, the call needs 16"):
        capi.mc_survival_dev(mc, i32[:8], 3, i32[:15])
    with pytest.raises(capi.F110QPError, match="crashed holds"):
        capi.mc_survival_dev(mc, i32[:8], 3, i32, i32[:3])
    with pytest.raises(capi.F110QPError, match=r"clear_traj must be \[T \+ 1, B\]"):
        capi.mc_outcomes_dev(t64[:8], t64)
    with pytest.raises(capi.F110QPError, match="status_traj holds"):
        capi.mc_outcomes_dev(v, t64, status_traj=i32[:15])
    with pytest.raises(capi.F110QPError, match="kind_traj must be torch.int32"):
        capi.mc_outcomes_dev(v, t64, kind_traj=t64)
    with pytest.raises(capi.F110QPError, match="need status_traj"):
        capi.mc_outcomes_dev(v, t64, unsolved=i32)
    with pytest.raises(capi.F110QPError, match="needs kind_traj"):
        capi.mc_outcomes_dev(v, t64, status_traj=i32, plan_failed=i32)
    with pytest.raises(capi.F110QPError, match="min_clear holds"):
        capi.mc_outcomes_dev(v, t64[:7])
    with pytest.raises(capi.F110QPError, match="min_row must be torch.int32"):
        capi.mc_outcomes_dev(v, t64, min_row=t64)
    clear, crash = np.zeros((3, 8)), np.zeros(8, np.int32)
    with pytest.raises(capi.F110QPError, match="float64"):
        capi.mc_summary(mc, clear.astype(np.float32), crash)
    with pytest.raises(capi.F110QPError, match=r"clear_traj must be \[T \+ 1, B\]"):
        capi.mc_summary(mc, np.zeros(8), crash)
    with pytest.raises(capi.F110QPError, match="crash_tick must be an int32"):
        capi.mc_summary(mc, clear, crash.astype(np.int64))
    with pytest.raises(capi.F110QPError, match="status_traj must be an int32"):
        capi.mc_summary(mc, clear, crash, status_traj=np.zeros((3, 8), np.int32))
    with pytest.raises(capi.F110QPError, match="must divide B = 8"):
        capi.mc_summary(capi.default_mc_config(hypotheses=3), clear, crash)
