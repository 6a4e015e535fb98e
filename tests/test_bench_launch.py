"""bench.py's rank launch (no GPU needed): `--gpus N` without a launcher starts N ranks itself
(RANK / LOCAL_RANK / WORLD_SIZE / 127.0.0.1 rendezvous), and under a launcher it refuses a
WORLD_SIZE that differs from --gpus. Both checks run before any GPU call."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _run(args, **env):
    e = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    e.update(env)
    return subprocess.run([sys.executable, BENCH] + args, env=e, capture_output=True, text=True, timeout=120)


def test_gpus_n_plans_n_ranks():
    r = _run(["--gpus", "4", "--config", "c4", "--print-launch"])
    assert r.returncode == 0, r.stderr
    plan = json.loads(r.stdout.strip().splitlines()[-1])
    assert [d["RANK"] for d in plan["ranks"]] == ["0", "1", "2", "3"]
    assert [d["LOCAL_RANK"] for d in plan["ranks"]] == ["0", "1", "2", "3"]
    assert {d["WORLD_SIZE"] for d in plan["ranks"]} == {"4"}
    assert {d["MASTER_ADDR"] for d in plan["ranks"]} == {"127.0.0.1"}
    assert len({d["MASTER_PORT"] for d in plan["ranks"]}) == 1
    # the children run this script with the same arguments (minus the test hook)
    assert plan["cmd"][1:] == [BENCH, "--gpus", "4", "--config", "c4"]


def test_world_size_mismatch_is_refused():
    r = _run(["--gpus", "2"], WORLD_SIZE="3", RANK="0", LOCAL_RANK="0")
    assert r.returncode == 2
    assert "refusing" in r.stderr


def test_gpus_zero_is_refused():
    r = _run(["--gpus", "0"])
    assert r.returncode == 2


def test_zero_steps_is_refused():
    r = _run(["--steps", "0"])
    assert r.returncode == 2
    assert "--steps" in r.stderr


def test_dump_outputs_writes_float32_and_samples_under_the_cap(tmp_path):
    """--dump-outputs: every array as <name>.npy in float32; above the byte cap the same seeded
    rows of every array, with their indices, identical from call to call."""
    import numpy as np

    sys.path.insert(0, ROOT)
    import bench

    B = 50
    u = np.arange(B * 6, dtype=np.float32).reshape(B, 3, 2)
    st = np.arange(B, dtype=np.int32)
    w = bench.dump_outputs(str(tmp_path / "all"), {"u": u, "status": st})
    assert w == {"u.npy": [B, 3, 2], "status.npy": [B]}
    got = np.load(tmp_path / "all" / "status.npy")
    assert got.dtype == np.float32 and np.array_equal(got, st)
    assert np.array_equal(np.load(tmp_path / "all" / "u.npy"), u)
    # 36 bytes per QP (24 + 4 + 8 for the index): a 360-byte cap keeps 10 QPs
    for d in ("s1", "s2"):
        w = bench.dump_outputs(str(tmp_path / d), {"u": u, "status": st}, suffix="_rank1", max_bytes=360)
        assert w["u_rank1.npy"] == [10, 3, 2] and w["sample_rows_rank1.npy"] == [10]
    rows = np.load(tmp_path / "s1" / "sample_rows_rank1.npy")
    assert rows.dtype == np.float64 and len(set(rows)) == 10 and np.all(np.diff(rows) > 0)
    assert np.array_equal(rows, np.load(tmp_path / "s2" / "sample_rows_rank1.npy"))
    assert np.array_equal(np.load(tmp_path / "s1" / "u_rank1.npy"), u[rows.astype(int)])
    assert np.array_equal(np.load(tmp_path / "s1" / "status_rank1.npy"), st[rows.astype(int)])
    total = sum(os.path.getsize(tmp_path / "s1" / f) - 128 for f in os.listdir(tmp_path / "s1"))
    assert total <= 360
