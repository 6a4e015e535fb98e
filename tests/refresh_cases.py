"""The refreshed-scan tests' CPU side (test_gpu_gap_refresh.py, test_gpu_rollout_refresh.py): hand-built scans
with the record each must give, the poses they are paired with, the gap record of a scan in numpy, and the
circle ahead of car 0 that opens the rollout's scene as a gap at row 0 and closes it a few ticks later."""
import numpy as np
import walls_cases as wl_
import world_cases as wc_
from halfspace_cases import closed_form, scan_geometry

NR = 1080
THRESH, DIVIDER, BUFFER = 3.0, 1.5, 3.0  # f110qp_default_scan_config


def window(nr=NR, divider=DIVIDER):
    """(first, last) beam inside the field-of-view window, with the kernel's float32 expressions."""
    amin, ainc, _ = scan_geometry(nr)
    f = np.float32
    lim = f(f(1.571) / f(divider))
    ang = (amin + np.arange(nr).astype(f) * ainc).astype(f)
    inside = np.flatnonzero((ang > -lim) & (ang < lim))
    return int(inside[0]), int(inside[-1])


def record(ranges, geom, thresh=THRESH, divider=DIVIDER, buffer=BUFFER):
    """(lo, hi) of f110qp_gap_search_dev for one scan: halfspace_cases.closed_form, then the buffer inflation of
    constraints.cpp:173-177 in float32."""
    lo, hi = closed_form(ranges, *geom, thresh=thresh, divider=divider)
    f = np.float32
    if f(hi - lo) > f(2.0) * f(buffer):
        hi, lo = int(f(hi) - f(buffer)), int(f(lo) + f(buffer))
    return lo, hi


def content_scans():
    """-> (ranges [S, 1080] float32, names, the (lo, hi) each must give)."""
    w0, w1 = window()
    mid = (w0 + w1) // 2
    out = []

    def add(name, want, fill=1.0):
        r = np.full(NR, fill, np.float32)
        out.append((name, r, want))
        return r

    add("no beam above the threshold", (-1, -1))
    r = add("single-beam gaps, the window opens on one", (0, 0))
    r[w0::2] = 5.0
    add("every beam open", (w0 + 3, w1 - 3), fill=5.0)
    r = add("a gap of 2 x buffer: not inflated", (mid, mid + 6))
    r[mid:mid + 7] = 5.0
    r = add("a gap one beam longer: inflated", (mid + 3, mid + 4))
    r[mid:mid + 8] = 5.0
    r = add("two runs of equal length: the first wins", (mid - 100 + 3, mid - 100 + 39 - 3))
    r[mid - 100:mid - 60] = 5.0
    r[mid + 60:mid + 100] = 5.0
    r = add("a gap touching the window's first beam", (w0 + 3, w0 + 49 - 3))
    r[:w0 + 50] = 5.0
    r = add("a gap touching the window's last beam", (w1 - 49 + 3, w1 - 3))
    r[w1 - 49:] = 5.0
    r = add("NaN splits a run, inf is open", (mid + 11 + 3, mid + 59 - 3))
    r[mid:mid + 60] = 5.0
    r[mid + 10] = np.nan
    r[mid + 30:mid + 40] = np.inf
    r = add("inf at both end beams after the inflation", (mid + 3, mid + 36))
    r[mid:mid + 40] = 5.0
    r[mid + 3], r[mid + 36] = np.inf, np.inf
    names, rs, want = zip(*out)
    return np.ascontiguousarray(np.stack(rs)), list(names), list(want)


def poses():
    """[P, 3] float64: the origin, headings round the circle, 1 km out with sub-float32 fractions, NaN poses."""
    rows = [[0.0, 0.0, 0.0]]
    rows += [[1.5, -2.25, a] for a in np.linspace(-np.pi, np.pi, 9)]
    far = np.float32([1000.0, -1000.0])
    frac = 0.3 * np.spacing(far).astype(np.float64)  # below the float32 ulp at 1 km
    rows += [[far[0] + frac[0], far[1] - frac[1], a] for a in (0.7, -2.9)]
    rows += [[np.nan, 0.0, 0.0], [0.0, 0.0, np.nan]]
    p = np.float64(rows)
    assert (p[10:12, :2].astype(np.float32).astype(np.float64) != p[10:12, :2]).all()
    return p


# ---- the rollout's scene ---------------------------------------------------------------------------------------

# metres from car 0's LiDAR at row 0 to the near face of the circle ahead, and its radius. The first tick is a
# PLAN tick (fail_u, 5 mm), a car without a path creeps at 5 mm a tick and one with a plan drives 45 mm a tick: over
# the five steps of T = 6 the car closes at least 25 mm, so the face starts 15 mm beyond ftg_thresh and ends at
# least 10 mm inside it, where the beams within sqrt(2 r 0.01) = 0.1 m of the axis (15 of them at 13 mm a beam)
# read below the threshold.
FACE, RADIUS = THRESH + 0.015, 0.5


def circle_ahead(x0, face=FACE, radius=RADIUS):
    """The circle (cx, cy, r) on the heading of pose x0 whose near face is `face` metres from the LiDAR."""
    c, s = np.cos(x0[2]), np.sin(x0[2])
    d = wc_.LIDAR_OFFSET + face + radius
    return np.float64([x0[0] + d * c, x0[1] + d * s, radius])


def oracle_record(x, circles, segments, G, geom, car=0):
    """The gap record (lo, hi) of one car's scan at the poses x [B, 3], from the numpy ray casts."""
    r = wl_.oracle_scan(np.ascontiguousarray(x, np.float64), circles, segments, G, geom, NR)
    return record(r[car], geom)
