"""bench.py's two modes: a plain run times the steps and prints the line (and, with --dump-outputs, writes the transcript of
its last timed step); --full adds everything reported beside the headline."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(args, timeout=600):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert r.returncode == 0 and lines, r.stdout[-2000:] + r.stderr[-2000:]
    return json.loads(lines[-1])


def _elements(bits):
    """float32 0/1 bit rows (least significant first) -> GF(2^128) elements as ints."""
    raw = np.packbits(bits.reshape(-1, 128).astype(np.uint8), axis=1, bitorder="little")
    return [int.from_bytes(row.tobytes(), "little") for row in raw]


def test_bench_rejects_a_step_count_below_one():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--steps" in r.stderr and not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]


@pytest.mark.gpu
def test_bench_plain_run_dumps_the_transcript_it_timed(oracle, tmp_path):
    import bench

    n_vars = 16
    out = tmp_path / "outputs"
    line = _bench(["--gpus", "1", "--steps", "3", "--warmup", "1", "--n-vars", str(n_vars), "--dump-outputs", str(out)])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["verifier_check"] is True
    # a plain run measures nothing beside the headline
    assert line["roofline"] is None and line["kernels"] is None and line["ms_per_step_instrumented"] is None
    assert "claim_groups" not in line and "cpu_baseline" not in line
    coeffs, finals = np.load(out / "round_coeffs.npy"), np.load(out / "final_evals.npy")
    assert sorted(os.listdir(out)) == ["final_evals.npy", "round_coeffs.npy"]
    assert coeffs.dtype == np.float32 and coeffs.shape == (n_vars, 3, 128)
    assert finals.dtype == np.float32 and finals.shape == (2, 128)
    assert set(np.unique(coeffs)) <= {0.0, 1.0} and set(np.unique(finals)) <= {0.0, 1.0}
    got_coeffs = [tuple(_elements(coeffs[r])) for r in range(n_vars)]
    got_finals = _elements(finals)
    assert bench.transcript_digest(got_coeffs, got_finals) == line["transcript_digest"]
    # ... and it is the oracle's transcript of bench.py's instance
    mls = [oracle.random_b128(0xB1A50000 + j, 1 << n_vars) for j in range(2)]
    rc, claim = oracle.inner_product(mls[0], 7, mls[1])
    assert rc == 0
    stream = oracle.random_scalars(0xC4A1, n_vars + 1)
    want_coeffs, want_finals = oracle.bivariate_sumcheck_prove(mls, n_vars, [(0, 1)], [claim], stream[0], stream[1:])
    assert got_coeffs == [tuple(c) for c in want_coeffs] and got_finals == list(want_finals)


@pytest.mark.gpu
def test_bench_full_reports_everything_beside_the_headline():
    line = _bench(["--gpus", "1", "--steps", "2", "--warmup", "1", "--n-vars", "16", "--full"])
    assert line["steps"] == 2 and line["verifier_check"] is True
    assert line["ms_per_step_instrumented"] > 0 and line["kernels"]
    assert line["roofline"]["kernel"] in line["kernels"] and line["roofline"]["measured_copy_GBps"] > 0
    assert set(line["claim_groups"]) == {"k4_m8", "k50_m100_keccak_width"}
    assert all(leg["verifier_check"] is True for leg in line["claim_groups"].values())
    assert line["cpu_baseline"]["value"] > 0
