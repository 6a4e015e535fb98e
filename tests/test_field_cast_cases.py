"""Rule F1's oracle held to rule G1's on the CPU (include/f110qp.h): workload.ray_field against workload.ray_grid
bit for bit on every beam of field_cast_cases.py, its visits against the rule taken literally (m single steps
between two reads of the field), and the count of cells it reads on the track map against the walk's. No GPU."""
import field_cast_cases as fcc
import numpy as np
import pytest

from f110qp import workload

CASES = fcc.cases()
RAW = fcc.raw_cases()


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def check(name, ox, oy, dx, dy, grid, cfg, max_range):
    d2 = fcc.field_of(grid)
    got, visits = workload.ray_field(ox, oy, dx, dy, d2, cfg, max_range)
    with np.errstate(invalid="ignore"):
        want = workload.ray_grid(ox, oy, dx, dy, grid, cfg, max_range)
    assert got.shape == want.shape == visits.shape and visits.dtype == np.int32
    assert (bits(got) == bits(want)).all(), (name, np.argwhere(bits(got) != bits(want))[:5])
    assert not np.signbit(got).any(), name
    single, count = fcc.each_beam(fcc.walk_field, ox, oy, dx, dy, d2, cfg, float(max_range))
    assert (bits(single) == bits(want)).all(), (name, "the m single steps")
    assert (visits == count).all(), (name, np.argwhere(visits != count)[:5])
    return got, visits


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.name)
def test_field_equals_walk(c):
    got, visits = check(c.name, *fcc.case_beams(c), c.grid, c.cfg, c.max_range)
    if c.name == "1x1 occupied":
        assert (got == 0).all() and (visits == 1).all()
    if c.name == "starts without a map":
        assert (got == c.max_range).all() and (visits == 0).all()
    if c.name == "empty map":
        assert (got == c.max_range).all() and (visits == 1).all(), "one jump, which leaves the map"
    if c.name.startswith("d2 "):
        d = int(c.name.split()[1])
        assert fcc.field_of(c.grid)[8, 8] == d
        assert (got[0] < c.max_range).any(), "some beam of the first car meets the cell"
    if c.name == "lattice, max_range 10.0":
        assert got[0, 0] == 0.875 and visits[0, 0] == 3, "a jump of three cells, then the step into the cell"
        assert got[1, 0] == 1.0 and (got[3] == 0).all() and (got[5] == 0).all()
    if c.name == "lattice, max_range 0.5":
        assert got[0, 0] == 0.5 and visits[0, 0] == 1, "max_range ends inside the first jump: no second read"
    if c.name == "lattice, max_range 0.875":
        assert got[0, 0] == 0.875 and visits[0, 0] == 3, "t == max_range is a hit"
    if c.name == "1x32768":
        assert got[0, 0] == (32767 - 0.5) * fcc.QUARTER and visits[0, 0] == 3, "one jump of 32,766 cells and a step"


@pytest.mark.parametrize("r", RAW, ids=lambda r: r.name)
def test_exact_beams(r):
    got, visits = check(r.name, r.ox, r.oy, r.dx, r.dy, r.grid, r.cfg, r.max_range)
    if r.name.startswith("corner wall"):
        assert (got < r.max_range).sum() >= 8, "the exact diagonals meet the wall at its corners"
    if r.name.startswith("1x32768"):
        assert got[0, 0] == (32767 - 0.5) * fcc.QUARTER and got[0, 4] == got[0, 0] and got[1, 0] == 0.0


def test_the_field_tells_occupied_cells():
    """d2 <= 0 is the rule's test of a cell: a field with negative entries reads as occupied there."""
    c = next(c for c in CASES if c.name == "lattice, max_range 10.0")
    d2 = fcc.field_of(c.grid)
    ox, oy, dx, dy = fcc.case_beams(c)
    want, _ = workload.ray_field(ox, oy, dx, dy, d2, c.cfg, c.max_range)
    got, _ = workload.ray_field(ox, oy, dx, dy, np.where(d2 == 0, -7, d2), c.cfg, c.max_range)
    assert (bits(got) == bits(want)).all()
    empty, visits = workload.ray_field(ox, oy, dx, dy, np.zeros((0, 0), np.int32), c.cfg, c.max_range)
    assert (empty == c.max_range).all() and (visits == 0).all()


def test_track_map_reads_a_quarter_of_the_cells():
    """make_grid_world(5, 40, 0.05), the map alone, 24 seeded free poses, every fourth of 1,080 beams: the field
    cast's reads of d2 are at most a quarter of the walk's reads of the map, the start cells included. (A jump that
    degenerated to single steps would read as many.)"""
    grid, cfg, d2, x, (ox, oy, dx, dy) = fcc.track()
    got, visits = workload.ray_field(ox, oy, dx, dy, d2, cfg, 10.0)
    want, reads = fcc.each_beam(fcc.walk_reads, ox, oy, dx, dy, grid, cfg, 10.0)
    assert (bits(got) == bits(want)).all()
    assert (bits(got) == bits(workload.ray_grid(ox, oy, dx, dy, grid, cfg, 10.0))).all()
    n = visits.size
    print(f"track map: {n} beams, field {visits.sum() / n:.2f} reads a beam, walk {reads.sum() / n:.2f}")
    assert n == fcc.TRACK_POSES * fcc.TRACK_BEAMS // fcc.TRACK_EVERY
    assert 4 * int(visits.sum()) <= int(reads.sum()), (int(visits.sum()), int(reads.sum()))
