"""The Monte Carlo outcomes' CPU side (test_mc_cases.py, test_gpu_mc.py): the cases whose device results are
compared with the numpy oracle (workload.mc_fan, mc_survival, mc_outcomes), and the comparison.

Comparison: bit for bit on every output. Every result is a selection or a count: a fan entry is one of the set's
own samples (its bits, so a zero's sign counts) or the one NaN 0x7ff8000000000000, which is compared by its bits
too. There is no tolerance and no skip rule.
"""
import numpy as np

from f110qp import workload

WAVE = 64          # the largest padded set of the wave kernel
GRID_WAVE = 2048   # mc_fan_grid's cap on the wave path: workgroups of four waves, 64 / P sets per wave
GRID_LDS = 1024    # and on the LDS path: one (row, set) per workgroup
PROB = (0.0, 0.05, 0.5, 0.95, 1.0)

# f110qp.h
SOLVED, SOLVED_INACCURATE, MAX_ITER, NO_SOLVE = 1, 2, 4, 0
TICK_MPC, TICK_PLAN, TICK_HOLD, TICK_PLAN_FAILED, TICK_CRASHED = 0, 1, 2, 3, 4


def same(got, want):
    """Equal shape, type and bits (NaN included)."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if got.dtype.kind == "f":
        return bool((got.view(np.uint64) == want.view(np.uint64)).all())
    return bool((got == want).all())


def check(name, got, want, what=""):
    """got: a dict of device results (an absent or None entry is an optional output left out)."""
    for k, w in want.items():
        g = got.get(k)
        if g is None:
            continue
        g = np.asarray(g).reshape(w.shape)
        if not same(g, w):
            gb, wb = (g.view(np.uint64), w.view(np.uint64)) if w.dtype.kind == "f" else (g, w)
            bad = np.argwhere(gb != wb)
            at = tuple(bad[0])
            raise AssertionError(f"{name} {what}: {k} differs at {len(bad)} of {w.size}, first {at} got {g[at]!r} "
                                 f"want {w[at]!r}")


def frozen(d):
    for v in d.values():
        v.setflags(write=False)
    return d


class FanCase:
    """v [rows, B] in sets of M at stride G, the quantiles prob."""

    def __init__(self, name, v, M, G=1, prob=PROB):
        self.name, self.M, self.G, self.prob = name, int(M), int(G), tuple(float(p) for p in prob)
        self.v = np.ascontiguousarray(v, np.float64)
        if self.v.ndim == 1:
            self.v = self.v[None]
        assert self.B % (self.M * self.G) == 0, (name, self.v.shape)
        self._oracle = None

    rows = property(lambda self: self.v.shape[0])
    B = property(lambda self: self.v.shape[1])
    K = property(lambda self: self.B // self.M)
    Q = property(lambda self: len(self.prob))

    def oracle(self):
        """dict of fan [rows, K, Q] and count [rows, K]: computed once, not to be written to."""
        if self._oracle is None:
            fan, count = workload.mc_fan(self.v, self.M, self.G, self.prob)
            self._oracle = frozen(dict(fan=fan, count=count))
        return self._oracle

    def check(self, got, what=""):
        check(self.name, got, self.oracle(), what)


def members(c, r, k):
    """The M values of set k at row r, read off the layout's own formula."""
    s, g = divmod(k, c.G)
    return c.v[r, [(s * c.M + m) * c.G + g for m in range(c.M)]]


# ---- fan cases -----------------------------------------------------------------------------------------------

SET_SIZES = (1, 2, 3, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1000, 4096)
STRIDES = tuple((G, M) for G in (2, 4, 7) for M in (5, 100))
ROWS = (1, 9)


def draws(rng, shape):
    """Normal values rounded to 1/8, so that a set of any size holds repeats, with a few large ones."""
    v = np.round(rng.normal(0.0, 4.0, shape) * 8.0) / 8.0
    return np.where(rng.random(shape) < 0.05, v * 1e9, v)


def size_case(M):
    S = 1 if M == 4096 else 2
    return FanCase(f"M={M}", draws(np.random.default_rng(500 + M), (2, S * M)), M)


def stride_case(G, M, S=3, rows=2):
    """v = 1e6 r + 1e4 s + 10 perm(m) + g: every value names the (r, s, m, g) it came from, and a set's minimum
    and maximum say which s and g it is."""
    perm = np.random.default_rng(600 + G + M).permutation(M)
    r, s, m, g = np.meshgrid(np.arange(rows), np.arange(S), np.arange(M), np.arange(G), indexing="ij")
    v = 1e6 * r + 1e4 * s + 10.0 * perm[m] + g
    return FanCase(f"G={G} M={M}", v.reshape(rows, S * M * G), M, G, (0.0, 0.5, 1.0))


def rows_case(rows, M=20):
    return FanCase(f"rows={rows}", draws(np.random.default_rng(700 + rows), (rows, 3 * M * 2)), M, 2)


def grid_cases():
    """rows x K past the grid cap of each path: the first waves (workgroups) take a second item. Wave path at
    M = 64 (one set per wave): 9 x 911 = 8,199 items > 2,048 x 4; LDS path at M = 65: 9 x 114 = 1,026 > 1,024."""
    a = FanCase("wave grid", draws(np.random.default_rng(801), (9, 911 * 64)), 64)
    b = FanCase("lds grid", draws(np.random.default_rng(802), (9, 114 * 65)), 65)
    assert a.rows * a.K > GRID_WAVE * 4 and b.rows * b.K > GRID_LDS
    return [a, b]


def packing_cases():
    """K no multiple of the sets packed into a wave: M = 3 pads to 4 (16 sets a wave) with K = 5 and rows = 3, so
    a wave holds sets of two rows and its last lanes none; M = 5 pads to 8 (8 a wave) with K = 3 x 7."""
    return [FanCase("K=5 of 16 a wave", draws(np.random.default_rng(811), (3, 15)), 3),
            FanCase("K=21 of 8 a wave", draws(np.random.default_rng(812), (2, 105)), 5, 7)]


NAN_POS = np.array([0x7FF8000000000000], np.uint64).view(np.float64)[0]
NAN_NEG = np.array([0xFFF8000000000000], np.uint64).view(np.float64)[0]
NAN_PAYLOAD = np.array([0x7FF00000DEADBEEF], np.uint64).view(np.float64)[0]   # a signalling NaN with a payload
NAN_NEG_PAYLOAD = np.array([0xFFFFFFFFFFFFFFFF], np.uint64).view(np.float64)[0]  # the pad key's own bits


def value_case(M):
    """One pattern per row, two situations (the second is the first shuffled, so the same fan): all equal; the
    special values; heavy duplicates; sorted; reversed; and NaN shares of none, some, all but one and all, with
    both NaN signs and payloads."""
    rng = np.random.default_rng(900 + M)
    special = np.array([0.0, -0.0, np.inf, -np.inf, 5e-324, -5e-324, 2.2250738585072014e-308, 1.0, -1.0,
                        1.7976931348623157e308])
    nans = np.array([NAN_POS, NAN_NEG, NAN_PAYLOAD, NAN_NEG_PAYLOAD])
    base = draws(rng, M)
    some = base.copy()
    some[rng.permutation(M)[:max(1, M // 3)]] = nans[np.arange(max(1, M // 3)) % 4]
    but_one = nans[np.arange(M) % 4].copy()
    but_one[M // 2] = -0.0
    rows = [np.full(M, 2.5), special[np.arange(M) % len(special)], rng.integers(0, 3, M).astype(np.float64),
            np.sort(base), np.sort(base)[::-1], base, some, but_one, nans[np.arange(M) % 4]]
    v = np.stack([np.concatenate([r, r[rng.permutation(M)]]) for r in rows])
    return FanCase(f"values M={M}", v, M)


def prob_cases():
    """Q = 1 and Q = 8; unsorted and repeated; {0, 1}; products with n - 1 that land on an integer (0.5 x 10,
    0.3 x 10 = 3 after rounding, 0.7 x 10 = 7.000000000000001) and just under one (the double below 0.5 times 10;
    0.29 x 100 = 28.999999999999996, 0.57 x 100 = 56.99999999999999)."""
    under = float(np.nextafter(0.5, 0.0))
    assert 0.29 * 100.0 < 29.0 and 0.57 * 100.0 < 57.0 and 0.3 * 10.0 == 3.0 and under * 10.0 < 5.0
    v11, v101 = draws(np.random.default_rng(1001), (2, 22)), draws(np.random.default_rng(1002), (2, 202))
    return [FanCase("Q=1", v11, 11, 1, (0.5,)),
            FanCase("Q=8 unsorted, repeated", v11, 11, 1, (1.0, 0.0, 0.5, 0.5, 0.25, 0.99, 0.0, 0.75)),
            FanCase("{0, 1}", v101, 101, 1, (0.0, 1.0)),
            FanCase("on and under an integer, n = 11", v11, 11, 1, (0.5, under, 0.3, 0.7)),
            FanCase("on and under an integer, n = 101", v101, 101, 1, (0.29, 0.57, 0.5, under))]


def fan_cases():
    c = [size_case(M) for M in SET_SIZES] + [stride_case(G, M) for G, M in STRIDES] + [rows_case(r) for r in ROWS]
    return c + grid_cases() + packing_cases() + [value_case(13), value_case(100)] + prob_cases()


# ---- survival cases ------------------------------------------------------------------------------------------

class SurvivalCase:
    def __init__(self, name, crash_tick, T, M, G=1):
        self.name, self.T, self.M, self.G = name, int(T), int(M), int(G)
        self.crash = np.ascontiguousarray(crash_tick, np.int32)
        self._oracle = None

    B = property(lambda self: self.crash.shape[0])
    K = property(lambda self: self.B // self.M)

    def oracle(self):
        if self._oracle is None:
            alive, crashed = workload.mc_survival(self.crash, self.T, self.M, self.G)
            self._oracle = frozen(dict(alive=alive, crashed=crashed))
        return self._oracle

    def check(self, got, what=""):
        check(self.name, got, self.oracle(), what)


def survival_case(M, G, T=6, S=8, seed=0):
    """Crash ticks drawn from -1, 0, a middle tick, T, T + 1, INT_MAX and -7 (every one at least once: B >= 8)."""
    B = S * M * G
    vals = np.array([-1, 0, T // 2, T, T + 1, np.iinfo(np.int32).max, -7])
    rng = np.random.default_rng(1100 + 10 * M + G + seed)
    ct = vals[np.concatenate([np.arange(len(vals)), rng.integers(0, len(vals), max(0, B - len(vals)))])[:B]]
    return SurvivalCase(f"survival M={M} G={G}", ct[rng.permutation(B)], T, M, G)


SURVIVAL = ((1, 1), (1, 4), (5, 1), (5, 4), (70, 1))


def survival_cases():
    return [survival_case(M, G) for M, G in SURVIVAL]


# ---- car records ---------------------------------------------------------------------------------------------

class OutcomesCase:
    def __init__(self, name, clear, status, kind):
        self.name = name
        self.clear = np.ascontiguousarray(clear, np.float64)
        self.status = np.ascontiguousarray(status, np.int32)
        self.kind = np.ascontiguousarray(kind, np.int32)
        self._oracle = {}

    T = property(lambda self: self.clear.shape[0] - 1)
    B = property(lambda self: self.clear.shape[1])

    def oracle(self, with_kind=True):
        """The records with kind_traj given, or NULL (every tick an MPC tick, no plan_failed)."""
        if with_kind not in self._oracle:
            self._oracle[with_kind] = frozen(workload.mc_outcomes(self.clear, self.status,
                                                                  self.kind if with_kind else None))
        return self._oracle[with_kind]

    def check(self, got, with_kind=True, what=""):
        check(self.name, got, self.oracle(with_kind), what)


def outcomes_case(T, B=70, seed=0):
    """Clearances with a tie on two rows (car 1: its minimum at rows 0 and T), a NaN row (row T // 2), an all-NaN
    column (car 2), +inf throughout (car 3), a -0 against a +0 (car 4: equal values, the lower row wins), NaN of
    both signs; kinds of every sort, HOLD and PLAN ticks carrying F110QP_NO_SOLVE, MPC ticks carrying every
    status."""
    rng = np.random.default_rng(1200 + T + seed)
    clear = rng.normal(1.0, 0.5, (T + 1, B))
    clear[T // 2] = np.where(np.arange(B) % 2 == 0, NAN_POS, NAN_NEG)
    clear[[0, T], 1] = -3.0
    clear[:, 2] = NAN_PAYLOAD
    clear[:, 3] = np.inf
    clear[:, 4] = 1.0
    clear[0, 4], clear[T, 4] = 0.0, -0.0
    kind = rng.choice([TICK_MPC, TICK_MPC, TICK_PLAN, TICK_HOLD, TICK_PLAN_FAILED, TICK_CRASHED], (T, B))
    status = np.where(kind == TICK_MPC, rng.choice([SOLVED, SOLVED, SOLVED_INACCURATE, MAX_ITER, 3, 5], (T, B)), NO_SOLVE)
    kind[:, 5], status[:, 5] = TICK_MPC, SOLVED                    # never unsolved
    kind[:, 6], status[:, 6] = TICK_HOLD, NO_SOLVE                 # unsolved only when kind_traj is NULL
    kind[:, 7], status[:, 7] = TICK_MPC, MAX_ITER                  # unsolved from tick 0 on
    return OutcomesCase(f"records T={T}", clear, status, kind)


OUTCOME_TICKS = (1, 12)


def outcomes_cases():
    return [outcomes_case(T) for T in OUTCOME_TICKS] + [outcomes_case(3, B=300, seed=1)]
