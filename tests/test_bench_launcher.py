"""bench.py --gpus N started WITHOUT a launcher must start its N ranks itself (the driver's contract; the fan-out the
reference does with its worker map, src/DomainDecomposition/DDParallel.jl:87-105,133-139)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _clean_env(**extra):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env.update(extra)
    return env


def test_launcher_refuses_more_ranks_than_gpus_unless_sharing_is_allowed():
    """No GPU initialised, no rank started: the parent only counts devices."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "64"], capture_output=True, text=True,
                       env=_clean_env(HIP_VISIBLE_DEVICES="0"), timeout=120)
    assert r.returncode != 0
    assert "only 1 GPU(s) visible" in (r.stderr + r.stdout)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["ghost", "halo"])
def test_bench_gpus2_from_a_bare_python_call(form):
    """Two fresh rank processes sharing the box's one GPU (host-staged plug-in transport), started by bench.py itself;
    rank 0's single JSON line comes back with n_gpus = 2 and (--full) the launcher's N = 1 reference - in the ghost-layer form
    (default: mg_ghost_*) and in the halo form of rounds 2-4 (mg_dist_*)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--cells", "32", "--steps", "3",
                        "--warmup", "1", "--sharded-form", form, "--full"], capture_output=True, text=True,
                       env=_clean_env(MG_BENCH_ALLOW_SHARE="1"),
                       timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip().startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 3 and out["scaling"] == "weak"
    assert out["launcher"]["ranks_started"] == 2 and out["launcher"]["shared_gpu"] is True
    assert out["n1_reference"]["value"] > 0 and out["parallel_efficiency_vs_n1"] is not None
    assert ("ghost layers" if form == "ghost" else "native C++ sequencer") in out["config"]["parallelism"]
    if form == "ghost":
        assert out["ghost"]["exchanges_per_step"] > 0 and out["transport"].startswith("plug-in")
    assert 0 < out["relres_after_steps"] < 1e-2


@pytest.mark.gpu
def test_bench_dump_outputs_are_the_timed_solve(mg, built, tmp_path):
    """--dump-outputs DIR: the residual history of exactly --steps steps and the iterate they produced (33^3 rows: x whole),
    which must leave the residual the history ends with on the seeded right-hand side bench.py solves."""
    K = 4
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--cells", "32", "--steps", str(K),
                        "--warmup", "1", "--no-cpu-baseline", "--no-generic-pass", "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, env=_clean_env(), timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.strip().startswith("{")][-1])
    assert out["steps"] == K and out["ms_per_step"] > 0
    assert sorted(os.listdir(tmp_path)) == ["resvec.npy", "x.npy"]
    resvec, x = np.load(tmp_path / "resvec.npy"), np.load(tmp_path / "x.npy")
    assert resvec.dtype == x.dtype == np.float64 and resvec.shape == (K + 1,) and x.shape == (33 ** 3,)
    assert resvec[-1] / resvec[0] == pytest.approx(out["relres_after_steps"], rel=1e-12)
    A, _ = mg.poisson_shifted([32, 32, 32])
    b = mg.seeded_rhs(A)
    assert abs(np.linalg.norm(b - A @ x) - resvec[-1]) <= 1e-10 * resvec[0]


@pytest.mark.gpu
def test_bench_plain_run_is_the_headline_and_full_adds_the_rest(built):
    """A plain run prints the headline line alone (roofline and cpu_baseline null); --full adds the instrumented per-kernel pass,
    the legs (at 32^3 cells: div sigma grad among them) and the CPU baseline after the same timed steps."""
    def run(*extra):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--cells", "32", "--steps", "4",
                            "--warmup", "1", *extra], capture_output=True, text=True, env=_clean_env(), timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.strip().startswith("{")]
        assert len(lines) == 1, r.stdout[-2000:]
        return json.loads(lines[0])

    plain, full = run(), run("--full")
    for out in (plain, full):
        assert out["metric"] == "V-cycle DoF-updates/s" and out["unit"] == "DoF-updates/s" and out["dtype"] == "f64"
        assert out["higher_is_better"] is True and out["steps"] == 4 and out["warmup"] == 1
        assert out["value"] > 0 and out["ms_per_step"] > 0 and len(out["timed_regions_ms_per_step"]) == 5
    assert plain["roofline"] is None and plain["cpu_baseline"] is None
    assert full["roofline"]["kernels"] and full["roofline"]["achieved"] > 0
    assert full["roofline"]["divsiggrad"]["ms_per_step"] > 0
    assert full["cpu_baseline"]["value"] > 0 and full["cpu_baseline"]["resvec_rel_diff_vs_gpu"] < 1e-10
    assert full["relres_after_steps"] == pytest.approx(plain["relres_after_steps"], rel=1e-10)
