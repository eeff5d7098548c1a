"""bench.py's command line: a plain run carries the headline figure alone (everything else is behind
--full), --steps sets the number of timed steps, and --dump-outputs writes what the last timed step
returned — bitwise what a caller of rmd.ops gets from the same seeded inputs."""

import json
import sys

import numpy as np
import pytest
import torch

# keys of the result line that only a --full run computes
FULL_ONLY = ("roofline", "roofline_gemm", "roofline_lookup", "fp32_mode", "model_level", "dicl_matching",
             "hybrid_inference", "train_step", "highres_fs", "cpu_baseline")


def _run_main(monkeypatch, capsys, *argv):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    bench.main()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_plain_dry_run_line_is_the_headline_alone(monkeypatch, capsys, tmp_path):
    res = _run_main(monkeypatch, capsys, "--gpus", "1", "--steps", "3", "--warmup", "1", "--dry-run",
                    "--dump-outputs", str(tmp_path / "out"))
    assert res["steps"] == 3 and res["warmup"] == 1 and res["ms_per_step"] > 0
    assert abs(res["value"] - 8 * 3 / (res["ms_per_step"] * 3 / 1e3)) < 1e-6 * res["value"]
    for key in ("metric", "unit", "higher_is_better", "dtype"):
        assert key in res
    assert not [k for k in FULL_ONLY if k in res]
    assert (tmp_path / "out").is_dir() and not list((tmp_path / "out").iterdir())     # a dry run computes nothing


def test_steps_must_be_positive(monkeypatch, capsys):
    with pytest.raises(SystemExit):
        _run_main(monkeypatch, capsys, "--gpus", "1", "--steps", "0", "--dry-run")


def test_dump_outputs_whole_or_fixed_sample_within_the_limit(monkeypatch, tmp_path):
    import bench
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4000)
    big = torch.arange(5000, dtype=torch.float64).reshape(50, 100)      # value = flat position
    small = torch.full((3, 4), 0.5, dtype=torch.float16)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "small": small}, 0, 1)
    a = np.load(tmp_path / "a" / "big.npy")
    s = np.load(tmp_path / "a" / "small.npy")
    assert a.dtype == np.float32 and s.dtype == np.float32
    assert s.shape == (3, 4) and (s == 0.5).all()                       # within its share: whole, own shape
    assert a.shape == (4000 // (4 * 2),)                                # over it: 1-D sample of the share's size
    assert (np.diff(a) > 0).all() and a[0] >= 0 and a[-1] < 5000        # distinct positions, ascending
    assert a.nbytes + s.nbytes <= 4000
    assert np.array_equal(a, np.load(tmp_path / "b" / "big.npy"))       # the same positions in every run
    bench.dump_outputs(str(tmp_path / "r"), {"big": big}, 1, 2)
    r = np.load(tmp_path / "r" / "big.rank1.npy")
    assert r.shape == (4000 // (4 * 2),)                                # two ranks share the limit


@pytest.mark.gpu
def test_plain_run_dumps_the_last_lookup_of_the_last_step(monkeypatch, capsys, tmp_path):
    """Small shape (16x24 feature maps, b2, C=64, bf16 mode): the dumped array is the 12th lookup of the
    pyramid of bench.synthetic's seeded inputs, bitwise."""
    import bench
    from rmd import ops
    res = _run_main(monkeypatch, capsys, "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "2",
                    "--channels", "64", "--height", "128", "--width", "192", "--dump-outputs", str(tmp_path))
    assert res["steps"] == 3 and res["ms_per_step"] > 0 and res["dtype"] == "bf16"
    assert abs(res["value"] - 2 * 3 / (res["ms_per_step"] * 3 / 1e3)) < 1e-6 * res["value"]
    assert not [k for k in FULL_ONLY if k in res]
    got = np.load(tmp_path / "corr_lookup_last.npy")
    assert got.dtype == np.float32 and got.shape == (2, 4 * 81, 16, 24)
    f1, f2, coords = bench.synthetic(2, 64, 16, 24, 12, 1234, torch.device("cuda", 0))
    want = ops.corr_lookup(ops.corr_pyramid(f1, f2, 4, "bf16"), coords[11], 4)
    assert np.array_equal(got, want.cpu().numpy())
    assert np.isfinite(got).all() and np.abs(got).max() > 0
