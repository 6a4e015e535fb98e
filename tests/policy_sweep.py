"""The sweep of launch-policy answers that tests/golden/launch_policy.rec records and
tests/test_launch_policy.py replays: which (config, test-build knob, horizon, batch) cases are asked, and
how. The introspection calls need no device.

A variant is a config corner plus at most one forced knob. Every config corner (gap rows x back end x
warm start x u_des[0] on / inside its speed bound x q[0] == / != q[1]) runs without a knob; every knob
value runs against gap rows off / on and back end AUTO / LANE at the default of the other axes."""
import itertools

HORIZONS = (1, 2, 3, 4, 5, 7, 8, 15, 16, 20, 21, 28, 29, 30, 32, 33, 40, 47, 48)
BATCHES = (1, 2, 8, 9, 63, 64, 65, 255, 256, 257, 512, 1023, 1024, 1025, 2048, 2049, 4096, 8192, 16384, 16385,
           32768, 32769, 65536, 131072)
KNOBS = (
    [("F110QP_LANE_SEG", v) for v in (1, 2, 4, 8)]
    + [("F110QP_LANE_SEG_F32", 1), ("F110QP_LANE_TWIN", 0), ("F110QP_SEG_FIXEDQ", 0), ("F110QP_LANE_DREF", 0),
       ("F110QP_LANE_ROT", 0)]
    + [("F110QP_LANE_QPW", v) for v in (1, 16, 64)]
    + [("F110QP_LANE_MODE", v) for v in (1, 2, 3, 4)]
    + [("F110QP_GAP_SCREEN", v) for v in (0, 1)]
)
KNOB_NAMES = sorted({k for k, _ in KNOBS})
# per (variant, horizon, batch): backend_info(B, grouped = False) and (B, grouped = True), three values
# each, then lane_segments, lane_starts, lane_fixed_q, gap_screen
ANSWERS = 10


def variants():
    """[{"gap", "backend", "warm", "udes_inside", "q_unequal", "knob": [name, value] or None}, ...]"""
    out = []
    for gap, backend, warm, ui, qn in itertools.product((0, 1), (0, 1, 2), (0, 1), (0, 1), (0, 1)):
        out.append(dict(gap=gap, backend=backend, warm=warm, udes_inside=ui, q_unequal=qn, knob=None))
    for (name, value), gap, backend in itertools.product(KNOBS, (0, 1), (0, 2)):
        out.append(dict(gap=gap, backend=backend, warm=0, udes_inside=0, q_unequal=0, knob=[name, value]))
    return out


def config(capi, v, horizon):
    over = dict(gap_mode=v["gap"], backend=v["backend"], warm_start=v["warm"])
    if v["udes_inside"]:
        over["u_des"] = [4.0, 0.0]  # strictly inside the shipped speed box [3.0, 4.5]
    if v["q_unequal"]:
        over["q"] = [10.0, 8.0, 0.0]
    return capi.default_config(horizon, **over)


def answers(capi, v):
    """The answers of variant v as a [len(HORIZONS)][len(BATCHES)][ANSWERS] list of ints. The caller has
    set v's knob in the environment (and no other of KNOB_NAMES); the solvers are the test build's."""
    out = []
    for n in HORIZONS:
        s = capi.Solver(config(capi, v, n), test_build=True)
        out.append([[*s.backend_info(b), *s.backend_info(b, grouped=True), s.lane_segments(b), s.lane_starts(b),
                     s.lane_fixed_q(b), int(s.gap_screen(b))] for b in BATCHES])
        s.close()
    return out
