"""The noisy ray cast on MI355X (f110qp_cast_scans_noisy_dev; include/f110qp.h rules Z1 and Z2) against
workload.noisy_scan applied to the device's own noise-free cast (f110qp_cast_scans_walls_dev): the noisy scan is a
pure function of the noise-free scan, so everything here is bit equality. The shapes are where the kernel can still
go wrong: the beam index across LDS tiles (1,300 beams), the car index under workgroup striding (520 cars) and under
a list, and the high halves of the 64-bit arithmetic."""
import noise_cases as nz
import numpy as np
import pytest
import walls_cases as wl_
import world_cases as wc_
from test_gpu_rollout import same_bits
from test_gpu_rollout_replan import dev
from test_gpu_rollout_scan import scan_config
from test_gpu_rollout_walls import B, G, scene
from test_gpu_walls import wall_cast, walls_of
from test_gpu_world_scan import SENTINEL

pytestmark = pytest.mark.gpu

SEED = 7


def noisy_cast(capi, cuda, x, static, segments, G, geom, beams, noise, tick, listed=None, count=None,
               off=wl_.CENTER_OFFSET):
    """f110qp_cast_scans_noisy_dev on host arrays into rows pre-filled with the sentinel -> ranges [B, R]."""
    import torch

    x = np.ascontiguousarray(x, np.float64)
    nb = x.shape[0]
    C = 0 if static is None else static.shape[-2]
    w = capi.default_world_config(num_circles=C, world_rows=1 if static is None or static.ndim == 2 else static.shape[0])
    race = capi.default_race_config(group_size=G, center_offset=off)
    wl = walls_of(capi, segments, nb)
    out = torch.full((nb, beams), float(SENTINEL), dtype=torch.float32, device=cuda)
    capi.cast_scans_noisy_dev(scan_config(capi, beams, geom), w, race, capi.default_body_config(), wl, noise, tick,
                              dev(cuda, x), dev(cuda, static) if C else None,
                              dev(cuda, segments) if wl.num_segments else None, out,
                              list_=None if listed is None else dev(cuda, np.asarray(listed, np.int32)),
                              count=None if listed is None else dev(cuda, np.int32([count])))
    torch.cuda.synchronize(cuda)
    return out.cpu().numpy()


@pytest.mark.parametrize("beams", [1080, 1300])
def test_against_its_own_noise_free_cast(capi, cuda, beams):
    """The rollout scene (B = 8, G = 2: mates, circles and 251 segments in the scans); 1,300 beams are two beam
    tiles of 1,152."""
    x0, _, circles, sg, _ = scene()
    assert x0.shape[0] == B == 8 and G == 2
    geom = wc_.geometry(beams)
    clean = wall_cast(capi, cuda, x0, circles, sg, G, geom, beams)
    hit = clean != np.float32(wc_.MAX_RANGE)
    assert (clean != SENTINEL).all() and hit.any(), "returns in the scene"
    same_bits(noisy_cast(capi, cuda, x0, circles, sg, G, geom, beams, capi.default_noise_config(), 3), clean,
              "the all-zero config is the walls cast")
    same_bits(noisy_cast(capi, cuda, x0, circles, sg, G, geom, beams,
                         capi.default_noise_config(seed=SEED, car_base=1000), 5), clean, "a seed alone is no noise")
    for tick in nz.TICKS:
        for base in nz.CAR_BASES:
            for setting in nz.SETTINGS:
                got = noisy_cast(capi, cuda, x0, circles, sg, G, geom, beams, nz.noise_config(capi, SEED, base, setting),
                                 tick)
                same_bits(got, nz.oracle(clean, SEED, base, tick, setting), f"tick {tick} car_base {base} {setting}")
                if setting[2] == 1.0:
                    assert (got == np.float32(wc_.MAX_RANGE)).all()
                else:
                    assert (got[hit] != clean[hit]).mean() > (0.5 if setting[2] == 0.0 else 0.05)
                    assert (got[~hit] == clean[~hit]).all()


def test_listed_mode(capi, cuda):
    c = wl_.tile_scan(40, C=5, G=1, B=8)
    noise = nz.noise_config(capi, SEED, 0, nz.SETTINGS[2])
    args = (c.x, c.static, c.segments, c.G, c.geom, c.beams, noise, 1)
    full = noisy_cast(capi, cuda, *args)
    same_bits(full, nz.oracle(wall_cast(capi, cuda, c.x, c.static, c.segments, c.G, c.geom, c.beams), SEED, 0, 1,
                              nz.SETTINGS[2]), "all cars")
    got = noisy_cast(capi, cuda, *args, listed=[5, 2, 7, 0, 0, 0, 0, 0], count=2)
    same_bits(got[[5, 2]], full[[5, 2]], "listed rows: the car's own stream, not the list slot's")
    assert (np.delete(got, [5, 2], axis=0) == SENTINEL).all(), "unlisted rows stay"
    none = noisy_cast(capi, cuda, *args, listed=[5, 2, 7, 0, 0, 0, 0, 0], count=0)
    assert (none == SENTINEL).all(), "count = 0 writes nothing"


def test_grid_stride(capi, cuda):
    """520 cars: past the cap of 512 workgroups, eight workgroups take a second car."""
    nb = 520
    c = wl_.tile_scan(9, C=5, G=1, B=nb)
    assert c.beams == 64
    clean = wall_cast(capi, cuda, c.x, c.static, c.segments, c.G, c.geom, c.beams)
    assert (clean < np.float32(wc_.MAX_RANGE)).any(axis=1).mean() > 0.9, "the cars have returns"
    got = noisy_cast(capi, cuda, c.x, c.static, c.segments, c.G, c.geom, c.beams,
                     nz.noise_config(capi, SEED, 0, nz.SETTINGS[2]), 2)
    same_bits(got, nz.oracle(clean, SEED, 0, 2, nz.SETTINGS[2]), "every car of 520")


def test_64_bit_halves(capi, cuda):
    c = wl_.tile_scan(40, C=5, G=1, B=8)
    seed, base = 2 ** 63 + 12345, 2 ** 32 + 7
    clean = wall_cast(capi, cuda, c.x, c.static, c.segments, c.G, c.geom, c.beams)
    got = noisy_cast(capi, cuda, c.x, c.static, c.segments, c.G, c.geom, c.beams,
                     nz.noise_config(capi, seed, base, nz.SETTINGS[2]), 5)
    same_bits(got, nz.oracle(clean, seed, base, 5, nz.SETTINGS[2]), "seed 2^63 + 12345, car_base 2^32 + 7")
    for other in ((seed - 2 ** 63, base), (seed, base - 2 ** 32)):  # the high halves are read
        assert (got != nz.oracle(clean, other[0], other[1], 5, nz.SETTINGS[2])).any(), other


def test_hypotheses(capi, cuda):
    """Eight identical poses, every car alone: eight different scans of one situation, and car_base shifts them."""
    c = wl_.tile_scan(40, C=5, G=1, B=8)
    x = np.ascontiguousarray(np.repeat(c.x[:1], 8, axis=0))
    setting = nz.SETTINGS[2]
    clean = wall_cast(capi, cuda, x, c.static, c.segments, 1, c.geom, c.beams)
    assert (clean.view(np.uint32) == clean[0].view(np.uint32)).all(), "one situation"
    a = noisy_cast(capi, cuda, x, c.static, c.segments, 1, c.geom, c.beams, nz.noise_config(capi, SEED, 0, setting), 0)
    assert all((a[i] != a[j]).any() for i in range(8) for j in range(i)), "pairwise different"
    b = noisy_cast(capi, cuda, x, c.static, c.segments, 1, c.geom, c.beams, nz.noise_config(capi, SEED, 1, setting), 0)
    same_bits(b[:7], a[1:], "car b at car_base 1 is car b + 1 at car_base 0")
