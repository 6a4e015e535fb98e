"""Cases and second formulations for the raster-map family (include/f110qp.h rules G1 and G2): small maps (at most
64 x 48 cells), a slab-test ray cast that shares nothing with the walk of workload.ray_grid, a brute-force
clearance over every occupied cell, and the poses the GPU tests aim at the kernel's edges."""
import numpy as np

from f110qp import workload

MAX_RANGE = 10.0
LIDAR_OFFSET = 0.275
CENTER_OFFSET = 0.1651
HL, HW = workload.HALF_LENGTH, workload.HALF_WIDTH
CORNER = 1e-9     # cells: a beam this close to a lattice corner may take either neighbour
AGREE = 1e-9      # metres: the walk against the slab test
SKIP_CAP = 0.01   # the share of beams the corner rule may leave out


def spec(grid, origin=(0.0, 0.0), resolution=0.1, reach=1.0):
    g = np.ascontiguousarray(grid, np.uint8)
    return g, workload.GridSpec(g.shape[1], g.shape[0], origin[0], origin[1], resolution, reach)


def room(W=40, H=30, resolution=0.1, origin=(0.0, 0.0), seed=0, blocks=6, reach=1.0):
    """A closed room: the border cells occupied, `blocks` random rectangles of cells inside, the middle kept free."""
    rng = np.random.default_rng(seed)
    g = np.zeros((H, W), np.uint8)
    g[0], g[-1], g[:, 0], g[:, -1] = 1, 1, 1, 1
    for _ in range(blocks):
        w, h = rng.integers(1, 5, 2)
        i, j = rng.integers(1, W - w), rng.integers(1, H - h)
        g[j:j + h, i:i + w] = 1
    g[H // 2 - 4:H // 2 + 4, W // 2 - 4:W // 2 + 4] = 0
    g[0], g[-1], g[:, 0], g[:, -1] = 1, 1, 1, 1
    return spec(g, origin, resolution, reach)


def free_poses(grid, cfg, B, seed, lidar_offset=LIDAR_OFFSET, yaws=None):
    """B poses whose LiDAR stands in a free cell of the map."""
    rng = np.random.default_rng(seed)
    H, W = grid.shape
    out = []
    while len(out) < B:
        yaw = rng.uniform(-np.pi, np.pi) if yaws is None else yaws[len(out) % len(yaws)]
        lx = cfg.origin_x + rng.uniform(0.0, W) * cfg.resolution
        ly = cfg.origin_y + rng.uniform(0.0, H) * cfg.resolution
        i, j = int(np.floor((lx - cfg.origin_x) / cfg.resolution)), int(np.floor((ly - cfg.origin_y) / cfg.resolution))
        if 0 <= i < W and 0 <= j < H and not grid[j, i]:
            out.append([lx - lidar_offset * np.cos(yaw), ly - lidar_offset * np.sin(yaw), yaw])
    return np.array(out)


def beams_of(x, geom, beams, lidar_offset=LIDAR_OFFSET):
    """(ox, oy [B, 1], dx, dy [B, R]) as the cast builds them (numpy's sincos)."""
    x = np.asarray(x, np.float64)
    ox, oy = x[:, 0] + lidar_offset * np.cos(x[:, 2]), x[:, 1] + lidar_offset * np.sin(x[:, 2])
    ang = x[:, 2:3] + (np.float64(geom[0]) + np.float64(geom[1]) * np.arange(beams, dtype=np.float64))[None, :]
    return ox[:, None], oy[:, None], np.cos(ang), np.sin(ang)


def slab_scan(ox, oy, dx, dy, grid, cfg, max_range=MAX_RANGE):
    """The second formulation of rule G1: the slab test of every beam against every occupied cell's box, the nearest
    entry parameter (0 for a start inside a box); a beam from outside the map sees nothing, as in the rule.
    Also the least distance, in cells, at which each beam passes a lattice corner of an occupied cell's box before
    its hit (the corner rule's measure)."""
    ox, oy, dx, dy = np.broadcast_arrays(ox, oy, dx, dy)
    H, W = grid.shape
    res = cfg.resolution
    px, py = (ox - cfg.origin_x) / res, (oy - cfg.origin_y) / res
    jj, ii = np.nonzero(grid)
    out = np.full(dx.shape, np.inf)
    near = np.full(dx.shape, np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        for i, j in zip(ii, jj):
            tx0, tx1 = (i - px) / dx * res, (i + 1 - px) / dx * res
            ty0, ty1 = (j - py) / dy * res, (j + 1 - py) / dy * res
            lox = np.where(dx == 0.0, np.where((px >= i) & (px < i + 1), -np.inf, np.inf), np.minimum(tx0, tx1))
            hix = np.where(dx == 0.0, np.where((px >= i) & (px < i + 1), np.inf, -np.inf), np.maximum(tx0, tx1))
            loy = np.where(dy == 0.0, np.where((py >= j) & (py < j + 1), -np.inf, np.inf), np.minimum(ty0, ty1))
            hiy = np.where(dy == 0.0, np.where((py >= j) & (py < j + 1), np.inf, -np.inf), np.maximum(ty0, ty1))
            lo, hi = np.maximum(lox, loy), np.minimum(hix, hiy)
            hit = (lo <= hi) & (hi >= 0.0)
            out = np.where(hit, np.minimum(out, np.maximum(lo, 0.0)), out)
            for cx, cy in ((i, j), (i + 1, j), (i, j + 1), (i + 1, j + 1)):  # the beam's distance to the corner
                along = (cx - px) * dx + (cy - py) * dy
                d = np.abs((cx - px) * dy - (cy - py) * dx)
                near = np.where(along >= -CORNER, np.minimum(near, d), near)
    inside = (px >= 0) & (px < W) & (py >= 0) & (py < H)
    out = np.where(inside, out, np.inf)
    return np.minimum(out, max_range), near


def visited_cells(ox, oy, dx, dy, t, cfg):
    """The cells a beam's points at the parameters t (metres) lie in."""
    x, y = ox + t * dx, oy + t * dy
    return (np.floor((x - cfg.origin_x) / cfg.resolution).astype(int),
            np.floor((y - cfg.origin_y) / cfg.resolution).astype(int))


def brute_clearance(x, grid, cfg, center_offset=CENTER_OFFSET, hl=HL, hw=HW):
    """Rule G2 without the window: every occupied cell of the map against every pose x [B, 3] -> (value [B],
    index j W + i [B]), +inf and -1 for an empty map."""
    x = np.asarray(x, np.float64)
    jj, ii = np.nonzero(grid)
    B = x.shape[0]
    if ii.size == 0:
        return np.full(B, np.inf), np.full(B, -1)
    c, s = np.cos(x[:, 2]), np.sin(x[:, 2])
    qx, qy = x[:, 0] + center_offset * c, x[:, 1] + center_offset * s
    v = workload.cell_body(ii[None, :], jj[None, :], cfg, qx[:, None], qy[:, None], c[:, None], s[:, None], hl, hw)
    v = np.where(np.isnan(v), np.inf, v)
    k = np.argmin(v, axis=1)
    return v[np.arange(B), k], jj[k] * grid.shape[1] + ii[k]


def write_pgm(path, pixels, binary=True, maxval=255, comment=True):
    """pixels [rows, cols] ints, top row first, as P5 or P2 (with a comment line in the header)."""
    p = np.asarray(pixels)
    head = f"{'P5' if binary else 'P2'}\n" + ("# a map\n" if comment else "") + f"{p.shape[1]} {p.shape[0]}\n{maxval}\n"
    with open(path, "wb") as f:
        f.write(head.encode())
        if binary:
            f.write(p.astype(np.uint8 if maxval < 256 else ">u2").tobytes())
        else:
            f.write("\n".join(" ".join(str(int(v)) for v in row) for row in p).encode() + b"\n")
