"""f110qp_gap_refresh_dev on MI355X: the records and the rows of the one launch are bit-identical to
f110qp_gap_search_dev followed by f110qp_half_space_rows_dev on the same inputs, at beam counts around the 64-beam
block, at 1,080, one past the 1,536-beam register batch (the re-read path) and in a third batch, for partial and
whole workgroups of four waves, on hand-built scans whose record is known, at poses at the origin, round the
circle, 1 km out and NaN. Every output starts as a marker and the rows beyond `batch` keep it."""
import numpy as np
import pytest
import refresh_cases as rf_
from halfspace_cases import scan_geometry
from test_gpu_rollout import bits, same_bits
from test_gpu_rollout_replan import dev
from test_gpu_rollout_scan import _scans, far_states, scan_config, split_rows

pytestmark = pytest.mark.gpu

GUARD = 3  # rows behind `batch` in both outputs


def gap_refresh(capi, cuda, st, r, geom, **kw):
    """f110qp_gap_refresh_dev on host arrays into outputs of B + GUARD marked rows -> (hs [B,2,3], records [B])."""
    import torch

    B, nr = r.shape
    gap = torch.full((B + GUARD, 4), -7, dtype=torch.int32, device=cuda)
    hs = torch.full((B + GUARD, 2, 3), -7.0, dtype=torch.float32, device=cuda)
    capi.gap_refresh_dev(scan_config(capi, nr, geom, **kw), dev(cuda, r), dev(cuda, st), gap, hs)
    torch.cuda.synchronize(cuda)
    gap, hs = gap.cpu().numpy(), hs.cpu().numpy()
    assert (gap[B:] == -7).all() and (hs[B:] == -7.0).all(), "a row beyond batch was written"
    return hs[:B], np.ascontiguousarray(gap[:B]).view(capi.GAP_RECORD_DTYPE).reshape(B)


def check(capi, cuda, st, r, geom, what, **kw):
    hs, rec = gap_refresh(capi, cuda, st, r, geom, **kw)
    hs2, rec2 = split_rows(capi, cuda, st, r, geom, **kw)
    same_bits(rec.view(np.int32), rec2.view(np.int32), what + ": records")
    same_bits(hs, hs2, what + ": rows")
    nr = r.shape[1]
    nogap = (rec["lo"] < 0) | (rec["hi"] < 0) | (rec["lo"] >= nr) | (rec["hi"] >= nr)
    assert np.isnan(rec["r_lo"][nogap]).all() and np.isnan(rec["r_hi"][nogap]).all() and np.isnan(hs[nogap]).all(), what
    return hs, rec


@pytest.mark.parametrize("nr", [1, 63, 64, 65, 1080, 1537, 3073])
def test_sizes(capi, cuda, nr):
    seen_gap = seen_none = False
    for B in (1, 3, 4, 5, 9):
        r, geom = _scans(B, nr, 50 + nr + B)
        d, _ = far_states(B, nr + B)
        _, rec = check(capi, cuda, d, r, geom, f"nr {nr} B {B}")
        seen_gap |= bool(((rec["lo"] >= 0) & (rec["hi"] > rec["lo"])).any())
        seen_none |= bool((rec["lo"] < 0).any())
    if nr >= 63:
        assert seen_gap and seen_none, "the sets hold a gap and a scan without one"


def test_a_gap_in_every_batch_of_a_long_scan(capi, cuda):
    """3,073 beams in a window that covers them all: the longest run lies in the first, the second or the third
    batch of 1,536 beams, or crosses from one into the next; the end ranges are re-read."""
    nr = 3073
    geom = (np.float32(-1.0), np.float32(2.0 / (nr - 1)), np.float32(1.0))
    runs = [(100, 400), (1600, 2000), (3060, 3073), (1500, 1580), (3000, 3073), (0, 3073)]
    r = np.full((len(runs), nr), 1.0, np.float32)
    for b, (s, e) in enumerate(runs):
        r[b, s:e] = 4.0 + 0.001 * np.arange(e - s, dtype=np.float32)  # every end range its own value
        r[b, 5:7] = 5.0  # a shorter run in the first batch
    d, _ = far_states(len(runs), 7)
    _, rec = check(capi, cuda, d, r, geom, "long scan")
    for b, (s, e) in enumerate(runs):
        lo, hi = rf_.record(r[b], geom)
        assert lo == s + 3 and hi in (e - 4, e - 5), "the fixture: the long run wins (its last beam may lie past num_scans)"
        assert (rec["lo"][b], rec["hi"][b]) == (lo, hi), (b, rec[b])
        assert rec["r_lo"][b] == r[b, lo] and rec["r_hi"][b] == r[b, hi], (b, rec[b])


def test_contents_and_poses(capi, cuda):
    """Every hand-built scan at every pose: the record is the one the scan was built for, whatever the pose; the
    rows are NaN exactly where the record has no gap, an end range is not finite or the pose is NaN."""
    scans, names, want = rf_.content_scans()
    poses = rf_.poses()
    S, P = len(scans), len(poses)
    r = np.ascontiguousarray(np.repeat(scans, P, axis=0))
    st = np.ascontiguousarray(np.tile(poses, (S, 1)))
    hs, rec = check(capi, cuda, st, r, scan_geometry(rf_.NR), "contents x poses")
    hs, rec = hs.reshape(S, P, 2, 3), rec.reshape(S, P)
    for i, name in enumerate(names):
        assert (rec["lo"][i] == want[i][0]).all() and (rec["hi"][i] == want[i][1]).all(), (name, rec[i, 0], want[i])
        if want[i][0] < 0:
            assert np.isnan(hs[i]).all(), name
            continue
        assert (bits(rec["r_lo"][i]) == bits(scans[i, want[i][0]])).all(), name
        assert (bits(rec["r_hi"][i]) == bits(scans[i, want[i][1]])).all(), name
        ends = np.isfinite(scans[i, list(want[i])]).all()
        finite = np.isfinite(poses).all(axis=1)
        assert np.isfinite(hs[i][finite]).all() == ends, name
        assert not np.isfinite(hs[i][~finite]).all(axis=(1, 2)).any(), name + ": a NaN pose gives NaN in its rows"
    assert (hs[2, 0] != hs[2, 1]).any(), "the rows follow the pose"


def test_other_scan_parameters(capi, cuda):
    """The threshold, the divider and the buffer reach the kernel: each moves the record, and the one launch still
    equals the two."""
    scans, _, _ = rf_.content_scans()
    d, _ = far_states(len(scans), 3)
    geom = scan_geometry(rf_.NR)
    base = check(capi, cuda, d, scans, geom, "defaults")[1]
    for kw in ({"ftg_thresh": 6.0}, {"divider": 3.0}, {"buffer": 1.0}, {"buffer": -3.0}):
        rec = check(capi, cuda, d, scans, geom, str(kw), **kw)[1]
        assert (rec.view(np.int32) != base.view(np.int32)).any(), kw
