"""First-contact insurance for the driver's multi-GPU bench: the N-rank command line of ``bench.py``
runs on every GPU test run -- all ranks on cuda:0, collectives through gloo (``--dry-run-one-gpu``: prints
``"dry_run": true``, never a measurement) -- and its ONE JSON line is parsed: the keys a scaling record is built from are
there, the work was sharded as ``dist.shard_bounds`` says, both forms of the reference means were timed.  No hardware
curve is asked of this test."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run_bench(*args, timeout=900):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True,
                       timeout=timeout, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.strip().splitlines() if ln.strip()]
    assert lines, p.stderr[-2000:]
    # the JSON line is the LAST line of stdout, and the only one that parses as the result object
    rec = json.loads(lines[-1])
    return rec, lines, p.stderr


@pytest.mark.parametrize("n_ranks", [2, 8])
def test_n_rank_command_line_dry_run(n_ranks):
    rec, lines, err = _run_bench("--gpus", str(n_ranks), "--dry-run-one-gpu", "--steps", "2", "--warmup", "1", "--full",
                                 "--no-e2e")
    assert rec["dry_run"] is True
    assert rec["n_gpus"] == n_ranks and rec["steps"] == 2 and rec["warmup"] == 1
    assert rec["unit"] == "cells/s" and rec["higher_is_better"] is True
    assert rec["value"] > 0 and rec["value_allreduce_means"] > 0 and rec["value_chained_means"] > 0
    assert rec["value_blocks_means"] > 0
    assert set(rec["forms"]) >= {"value", "value_allreduce_means", "value_chained_means", "value_blocks_means"}
    assert "integer blocks" in rec["forms"]["value"]
    # `value` is the faster of the two exact forms of the means
    assert rec["value"] == pytest.approx(max(rec["value_blocks_means"], rec["value_chained_means"]), rel=1e-9)
    per_gpu = rec["config"]["cells_per_gpu"]
    assert len(per_gpu) == n_ranks and sum(per_gpu) == rec["config"]["cells_total"]
    assert all(c % 5000 == 0 for c in per_gpu[:-1])  # chunk-aligned shards
    assert rec["roofline"]["bound"] == "hbm" and 0 < rec["roofline"]["frac"] < 1.5
    assert "gloo" in rec["config"]["parallelism"]
    # the digest is the last key of the line (what survives a truncated record) and repeats the headline
    assert list(rec)[-1] == "summary"
    assert rec["summary"]["value_cells_per_s"] == round(rec["value"], 0)


def test_one_gpu_line_ends_with_json_and_warns_once():
    """N = 1 at a reduced size: the JSON line is the last line of stdout, the digest is its last key, and the
    reference's "Using mean of all cells" warning appears once in the process output, not once per call."""
    rec, lines, err = _run_bench("--steps", "3", "--warmup", "1", "--cells", "20000", "--full", "--no-cpu-baseline",
                                 "--no-e2e", "--no-extra")
    assert rec["n_gpus"] == 1 and rec["steps"] == 3 and rec["value"] > 0
    assert rec["roofline"]["kernel_ms"] > 0 and "stages" in rec
    assert list(rec)[-1] == "summary"
    assert err.count("Using mean of all cells as reference") <= 1
    assert "bench-summary " in err


def _dump(d):
    import numpy as np

    files = sorted(os.listdir(d))
    assert files and all(f.endswith(".npy") for f in files), files
    assert sum(os.path.getsize(os.path.join(d, f)) for f in files) <= 64 << 20
    arrays = {f[:-4]: np.load(os.path.join(d, f)) for f in files}
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    return arrays


def test_plain_line_is_lean_and_dumps_reproducible_outputs(tmp_path):
    """A plain N = 1 run times the headline step only (no legs of --full in the line), and --dump-outputs writes the
    last step's X_cnv; a second run with the same arguments writes the same arrays, and the N-rank path (2 ranks on one
    GPU) writes the same rows of X_cnv, shard by shard."""
    import numpy as np

    runs = []
    for k in range(2):
        rec, _, _ = _run_bench("--steps", "3", "--warmup", "1", "--cells", "20000", "--dump-outputs",
                               str(tmp_path / f"n1_{k}"))
        assert rec["steps"] == 3 and rec["ms_per_step"] > 0 and rec["value"] > 0
        assert rec["unit"] == "cells/s" and rec["higher_is_better"] is True and rec["dtype"] == "f64"
        assert not {"stages", "cpu_baseline", "e2e", "extra", "scale_n1"} & set(rec)
        runs.append(_dump(tmp_path / f"n1_{k}"))
    a, b = runs
    assert set(a) == set(b) >= {"x_cnv_rows", "x_cnv_row_index", "x_cnv_row_sum", "x_cnv_row_nnz", "chr_pos"}
    for name in a:
        np.testing.assert_array_equal(a[name], b[name], err_msg=name)
    assert a["x_cnv_row_sum"].shape == (20000,) and a["x_cnv_rows"].shape[0] == a["x_cnv_row_index"].shape[0]
    assert np.all(np.diff(a["x_cnv_row_index"]) > 0) and a["x_cnv_row_nnz"].sum() > 0

    rec, _, _ = _run_bench("--gpus", "2", "--dry-run-one-gpu", "--steps", "2", "--warmup", "1", "--cells", "20000",
                           "--dump-outputs", str(tmp_path / "n2"))
    assert "value_allreduce_means" not in rec and "e2e" not in rec
    c = _dump(tmp_path / "n2")
    np.testing.assert_array_equal(np.concatenate([c["x_cnv_row_nnz.rank0"], c["x_cnv_row_nnz.rank1"]]),
                                  a["x_cnv_row_nnz"])
    np.testing.assert_array_equal(np.concatenate([c["x_cnv_row_sum.rank0"], c["x_cnv_row_sum.rank1"]]),
                                  a["x_cnv_row_sum"])
    np.testing.assert_array_equal(c["chr_pos.rank0"], a["chr_pos"])
