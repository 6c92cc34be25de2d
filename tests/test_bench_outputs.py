"""bench.py --dump-outputs and the plain / --full split: the files hold what the timed path returned
(float32 / float64, under 64 MB, the gradient as a fixed sample of whole rows), two runs with the
same arguments write the same files, and a plain run's line carries the headline figures only."""

import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
NAMES = ["dlogits_sample.npy", "dlogits_sample_rows.npy", "loss.npy", "rows.npy", "stats.npy"]


def test_dump_outputs_samples_whole_gradient_rows(tmp_path):
    sys.path[:0] = [str(ROOT)]
    import bench

    T, V = 300, 1 << 16  # 4 V bytes x 300 rows > the sample's budget: 192 rows are kept
    g = torch.Generator().manual_seed(0)
    dlogits = torch.randn((1, T, V), generator=g).to(torch.bfloat16)
    last = {"loss": torch.tensor(1.5, requires_grad=True), "stats": torch.arange(5, dtype=torch.float64),
            "rows": torch.randn((8, T - 1), generator=g)}
    bench.dump_outputs(tmp_path / "a", last, dlogits)
    bench.dump_outputs(tmp_path / "kept", last, dlogits, stats_keep=[0, 1, 3])
    assert np.load(tmp_path / "kept" / "stats.npy").tolist() == [0.0, 1.0, 3.0]
    bench.dump_outputs(tmp_path / "b", last, dlogits)
    got = {n[:-4]: np.load(tmp_path / "a" / n) for n in NAMES}
    assert sorted(p.name for p in (tmp_path / "a").iterdir()) == NAMES
    assert sum(x.nbytes for x in got.values()) <= 64 << 20
    assert all(x.dtype in (np.float32, np.float64) for x in got.values())
    picked = got["dlogits_sample_rows"].astype(np.int64)
    assert len(picked) == bench.DUMP_SAMPLE_BYTES // (4 * V) == 192 and len(set(picked)) == 192
    assert picked.min() >= 0 and picked.max() < T and np.all(np.diff(picked) > 0)
    assert np.array_equal(got["dlogits_sample"], dlogits[0].float().numpy()[picked])
    assert got["loss"].tolist() == [1.5] and np.array_equal(got["stats"], np.arange(5.0))
    assert np.array_equal(got["rows"], last["rows"].numpy())
    for n in NAMES:  # the same sample every time
        assert np.array_equal(got[n[:-4]], np.load(tmp_path / "b" / n))


@pytest.mark.gpu
def test_plain_run_is_lean_and_its_dump_repeats(tmp_path):
    lines = []
    for d in ("a", "b"):
        r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                            "--tokens", "4096", "--dump-outputs", str(tmp_path / d)],
                           capture_output=True, text=True, timeout=120, cwd=tmp_path)
        assert r.returncode == 0, r.stderr[-2000:]
        out = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(out) == 1, r.stdout[-2000:]
        lines.append(json.loads(out[0]))
    line = lines[0]
    assert line["steps"] == 3 and line["warmup"] == 1 and line["full"] is False
    assert line["unit"] == "tokens/s" and line["higher_is_better"] is True and line["dtype"] == "bf16"
    assert line["ms_per_step"] > 0
    assert abs(line["value"] - 4096 / line["ms_per_step"] * 1e3) <= 2e-3 * line["value"]  # both are rounded
    assert line["roofline"]["kernel_ms"] > 0 and line["roofline"]["box_copy"] is None
    assert line["cpu_baseline"] is None and line["probe_wall_s"] == {}
    assert not {"c3_dp", "c3_dp_value_head", "trainer_step", "loss_head_fp32", "snapshot_overlap"} & set(line)
    a = {n[:-4]: np.load(tmp_path / "a" / n) for n in NAMES}
    assert sorted(p.name for p in (tmp_path / "a").iterdir()) == NAMES
    assert sum(x.nbytes for x in a.values()) <= 64 << 20
    assert all(x.dtype in (np.float32, np.float64) for x in a.values())
    assert a["dlogits_sample"].shape == (len(a["dlogits_sample_rows"]), 151936) and a["rows"].shape == (8, 4095)
    assert a["loss"][0] == np.float32(-a["stats"][0])
    assert a["stats"].shape == (34,)  # the 39 slots less the five that only a value head fills
    assert all(np.isfinite(x).all() for x in a.values()) and np.count_nonzero(a["dlogits_sample"]) > 0
    for n in NAMES:  # seeded inputs, deterministic kernels: output for output
        assert np.array_equal(a[n[:-4]], np.load(tmp_path / "b" / n), equal_nan=True), n
