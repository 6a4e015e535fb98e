"""The noisy LiDAR's rule without a GPU (include/f110qp.h rules Z1 and Z2; workload.scan_noise_draws and
workload.noisy_scan, the oracle of test_gpu_noise.py): the known answers, the moments and the independence of the
draws over 16 cars x 8 ticks x 1,080 beams at seed 7, and the properties of rule Z2."""
import os

import noise_cases as nz
import numpy as np

from f110qp import workload

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_known_answers():
    h, g, d = workload.scan_noise_draws(nz.KNOWN_SEED, 0, 0, 4)
    assert h.dtype == np.uint64 and tuple(int(v) for v in h) == nz.KNOWN_H
    assert tuple(int(v) for v in g) == nz.KNOWN_G
    assert tuple(int(v) for v in d) == nz.KNOWN_D
    assert workload.NOISE_U.hex() == nz.U_HEX
    assert workload.NOISE_U == float(np.float64(np.sqrt(np.float64(3.0) / np.float64(2 ** 32 - 1))))
    hdr = open(os.path.join(ROOT, "include", "f110qp.h")).read()
    assert nz.U_HEX in hdr and all(f"{v:#018x}" in hdr for v in nz.KNOWN_H), "the header states the same answers"
    # the beam index is the beam's index in the whole scan: a longer scan starts with the shorter one
    assert (workload.scan_noise_draws(nz.KNOWN_SEED, 0, 0, 1300)[0][:4] == h).all()


def test_moments():
    g, d = nz.block()
    z = g.astype(np.float64) * workload.NOISE_U
    print(f"mean {z.mean():.4f} std {z.std():.4f} max {np.abs(z).max():.4f}")
    assert abs(z.mean()) < 0.02
    assert abs(z.std() - 1.0) < 0.02
    assert np.abs(z).max() <= nz.G_MAX and 131070 * workload.NOISE_U <= nz.G_MAX
    assert np.abs(g).max() <= 131070
    assert int(d.max()) < 2 ** 24
    share = float((d < np.uint64(int(np.floor(0.1 * 2 ** 24)))).mean())
    print(f"dropout share {share:.4f}")
    assert abs(share - 0.1) < 0.01


def test_independence():
    g, _ = nz.block(cars=2, ticks=2)
    beams = nz.corr(g[0, 0, :-1], g[0, 0, 1:])  # 1,079 pairs of neighbours
    cars = nz.corr(g[0, 0], g[1, 0])
    ticks = nz.corr(g[0, 0], g[0, 1])
    print(f"correlation: neighbouring beams {beams:.3f}, car 0 / car 1 {cars:.3f}, tick 0 / tick 1 {ticks:.3f}")
    assert abs(beams) < 0.15 and abs(cars) < 0.15 and abs(ticks) < 0.15


def scans(B=6, R=1080, seed=3):
    """Noise-free scans with every kind of beam: returns between 0.05 and 9.9 m and a fifth without a return."""
    rng = np.random.default_rng(seed)
    r = rng.uniform(0.05, 9.9, (B, R)).astype(np.float32)
    r[rng.random((B, R)) < 0.2] = np.float32(10.0)
    return r


def test_zero_config_is_the_identity():
    r = scans()
    out = workload.noisy_scan(r, 99, 5, 3, 0.0, 0.0, 0.0)
    assert out.dtype == np.float32 and (out.view(np.uint32) == r.view(np.uint32)).all()


def test_no_return_is_untouched_and_dropout_one_drops_all():
    r = scans()
    none = r == np.float32(10.0)
    assert none.any() and (~none).any()
    for s in nz.SETTINGS + ((5.0, 1.0, 0.5),):
        assert (nz.oracle(r, 7, 0, 2, s)[none] == np.float32(10.0)).all(), s
    assert (workload.noisy_scan(r, 7, 0, 2, 0.3, 0.1, 1.0) == np.float32(10.0)).all()
    some = workload.noisy_scan(r, 7, 0, 2, 0.0, 0.0, 0.1)
    dropped = (some == np.float32(10.0)) & ~none
    assert 0.05 < dropped.sum() / (~none).sum() < 0.15 and (some[~dropped] == r[~dropped]).all()
    # another max_range: its own float is the no-return value
    r30 = np.where(none, np.float32(30.0), r)
    assert (workload.noisy_scan(r30, 7, 0, 2, 0.3, 0.1, 0.0, 30.0)[none] == np.float32(30.0)).all()


def test_the_result_stays_in_range():
    r = scans()
    out = workload.noisy_scan(r, 7, 0, 0, 5.0, 1.0, 0.0)  # sigma of 5 to 15 m: clamps both ways
    assert (out >= 0).all() and (out <= np.float32(10.0)).all()
    hit = r != np.float32(10.0)
    assert (out[hit] == 0).any() and (out[hit] == np.float32(10.0)).any() and ((out[hit] > 0) & (out[hit] < 10)).any()
    mild = workload.noisy_scan(r, 7, 0, 0, 0.01, 0.0, 0.0)
    assert (np.abs(mild.astype(np.float64) - r)[hit] <= 0.01 * nz.G_MAX + 1e-6).all(), "the noise is bounded"
    assert (mild[hit] != r[hit]).mean() > 0.9


def test_deterministic_and_keyed():
    r = scans()
    a = workload.noisy_scan(r, 7, 0, 0, 0.05, 0.01, 0.1)
    assert (a.view(np.uint32) == workload.noisy_scan(r.copy(), 7, 0, 0, 0.05, 0.01, 0.1).view(np.uint32)).all()
    assert (a != workload.noisy_scan(r, 8, 0, 0, 0.05, 0.01, 0.1)).any(), "seed"
    assert (a != workload.noisy_scan(r, 7, 1, 0, 0.05, 0.01, 0.1)).any(), "car"
    assert (a != workload.noisy_scan(r, 7, 0, 1, 0.05, 0.01, 0.1)).any(), "tick"
    same = np.repeat(r[:1], 4, axis=0)  # one scan four times: four different hypotheses
    b = workload.noisy_scan(same, 7, 0, 0, 0.05, 0.01, 0.1)
    assert all((b[i] != b[j]).any() for i in range(4) for j in range(i))


def test_car_base_shifts_the_stream():
    r = scans()
    same = np.repeat(r[:1], 6, axis=0)
    for k in (1, 3, 2 ** 32 + 7):
        a = workload.noisy_scan(same[:3], 7, k, 4, 0.05, 0.01, 0.1)
        b = workload.noisy_scan(same[:3], 7, 0, 4, 0.05, 0.01, 0.1) if k > 3 else None
        if k <= 3:
            full = workload.noisy_scan(same, 7, 0, 4, 0.05, 0.01, 0.1)
            assert (a.view(np.uint32) == full[k:k + 3].view(np.uint32)).all(), k
        else:
            h0 = workload.scan_noise_draws(7, k, 4, 8)[0]
            assert (h0 != workload.scan_noise_draws(7, 7, 4, 8)[0]).all(), "the high half of the car index is read"
            assert (a != b).any()
