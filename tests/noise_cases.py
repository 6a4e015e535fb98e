"""The noisy-LiDAR tests' CPU side (test_noise_cases.py, test_gpu_noise.py, test_gpu_rollout_noisy.py): the known
answers of rule Z1 (include/f110qp.h), the draws of a block of cars and ticks, the settings the device tests run and
the oracle call they share."""
import numpy as np

from f110qp import workload

# rule Z1's known answers: seed 1234, car_base + b = 0, t = 0, beams 0 to 3
KNOWN_SEED = 1234
KNOWN_H = (0x52b6d2127195ace2, 0x47208de8f3630884, 0x4c2edc5013e0a4f2, 0x8f2930e8f7aeddb0)
KNOWN_G = (17217, -12047, -7854, 38257)
KNOWN_D = (5026570, 3948636, 15546533, 623436)
U_HEX = "0x1.bb67ae86627e8p-16"
G_MAX = 3.4642  # |g U| never exceeds it: 131070 U = 3.46413...

# (sigma_abs, sigma_rel, dropout) of the device tests
SETTINGS = ((0.01, 0.0, 0.0), (0.0, 0.02, 0.0), (0.05, 0.01, 0.1), (0.0, 0.0, 1.0))
TICKS = (0, 1, 5)
CAR_BASES = (0, 1000)


def block(seed=7, cars=16, ticks=8, beams=1080):
    """(g [cars, ticks, beams] int64, d [cars, ticks, beams] uint64) of rule Z1."""
    g = np.empty((cars, ticks, beams), np.int64)
    d = np.empty((cars, ticks, beams), np.uint64)
    for c in range(cars):
        for t in range(ticks):
            _, g[c, t], d[c, t] = workload.scan_noise_draws(seed, c, t, beams)
    return g, d


def corr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.corrcoef(a, b)[0, 1])


def oracle(clean, seed, car_base, tick, setting, max_range=10.0):
    """workload.noisy_scan of the noise-free scans clean [B, R] at one of SETTINGS."""
    sa, sr, dr = setting
    return workload.noisy_scan(clean, seed, car_base, tick, sa, sr, dr, max_range)


def noise_config(capi, seed, car_base, setting):
    sa, sr, dr = setting
    return capi.default_noise_config(seed=seed, car_base=car_base, sigma_abs=sa, sigma_rel=sr, dropout=dr)
