"""-m gpu: the two driver entry points as the driver runs them -- `python bench.py` (one JSON line with the contract's
keys) and `__graft_entry__.smoke()` -- each in its own process (bench.py imports torch before the library)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def check_roofline(d):
    """`roofline.frac` is a fraction of a roof the kernel can actually hit: in (0, 1], = achieved / peak, for whichever
    kernel ran -- the on-chip CG is priced in algorithmic flops against the fp64 vector peak, the streaming kernels in
    the bytes a fused iteration must move against the HBM peak."""
    rf = d["roofline"]
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-12 and 0.0 < rf["frac"] <= 1.0, rf
    assert "traffic" in rf
    if d["config"]["cg_kernel"] == 2:
        assert rf["bound"] == "valu-fp64" and rf["unit"] == "TFLOP/s" and rf["peak"] == 78.65
        if rf.get("counted"):
            assert 0.0 < rf["counted"]["valu_busy"] <= 1.0 and 0.0 < rf["counted"]["hbm_frac_live"] <= 1.0
    else:
        assert rf["bound"] == "hbm" and rf["unit"] == "GB/s" and rf["peak"] == 8000.0
    # the line vouches for its own solution: true residual |f - K u| / |b| at about the stop tolerance, on every rank
    assert d["verify"]["ok_on_every_rank"] is True and 0.0 < d["verify"]["rel_true_residual"] <= d["verify"]["bar"]
    sp = d["spmv"]
    assert sp["bound"] == "hbm" and 0.0 < sp["frac"] <= 1.0 and abs(sp["frac"] - sp["achieved"] / sp["peak"]) < 1e-12


def test_bench_default_config_roofline_is_a_fraction(built):
    """the DEFAULT line (hole1m, on-chip kernel) -- what the driver records as BENCH: frac in (0, 1]"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1", "--warmup", "1",
                        "--full", "--no-cpu-baseline", "--no-hbm-resident", "--op-reps", "50"],
                       cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0])
    assert d["config"]["cg_kernel"] == 2 and d["fallback"] is False and d["cg_iterations"] == 5389
    check_roofline(d)
    # profiles/pmc_summary.json: counters of THIS build of the kernels ride along, those of another build are flagged
    assert d["roofline"]["traffic"] > 0 and isinstance(d["roofline"]["traffic_stale"], bool)
    assert (d["roofline"]["counted"] is None) == d["roofline"]["traffic_stale"]


def test_bench_prints_one_contract_line(built):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "plate100k", "--steps", "2",
                        "--warmup", "1", "--full", "--cpu-sample-iters", "20", "--op-reps", "50"],
                       cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in d, key
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1
    assert d["unit"] == "elements/s" and d["higher_is_better"] is True and d["scaling"] == "weak"
    assert d["vs_baseline"] is None and d["dtype"] == "f64" and d["data"] == "synthetic"
    assert "workload" in d["config"] and "model" not in d["config"]
    assert d["value"] > 0 and abs(d["value"] - d["config"]["elements"] / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
    check_roofline(d)
    # the HBM-resident leg: the same kernels on the 16M-triangle mesh, beyond the 256 MiB Infinity Cache
    hr = d["hbm_resident"]
    assert hr["elements"] > 15_000_000
    for leg in ("spmv", "iteration"):
        k = hr[leg]
        assert k["bound"] == "hbm" and k["peak"] == 8000.0 and not k["working_set_fits_infinity_cache"]
        assert abs(k["frac"] - k["achieved"] / k["peak"]) < 1e-12 and 0.0 < k["frac"] <= 1.0
    assert hr["spmv"]["frac"] >= 0.40                # north_star: >= 40 % of peak HBM bandwidth in the CG SpMV
    assert d["fallback"] is False
    cb = d["cpu_baseline"]
    assert cb["kind"] == "port" and cb["cores"] == 1 and cb["unit"] == "elements/s" and cb["value"] > 0 and cb["sample"]
    assert d["value"] > 10.0 * cb["value"]          # north_star: >= 10x the CPU solver at 1 GPU


def test_bench_plain_run_is_lean_and_dumps_what_it_returned(built, tmp_path):
    """Without --full the line holds the headline and the library's statistics, nothing measured after the steps;
    --dump-outputs writes what the last timed step returned (u, f, stress) in float64."""
    import numpy as np

    import bench
    out = tmp_path / "outputs"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "plate100k", "--steps", "3",
                        "--warmup", "1", "--dump-outputs", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["cg_converged"] == 1
    assert d["unit"] == "elements/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert abs(d["value"] - d["config"]["elements"] / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
    for key in ("roofline", "spmv", "verify", "hbm_resident", "unstructured", "cpu_baseline"):
        assert key not in d, key
    prob, _ = bench.build_problem("plate100k", 1)
    N, E = prob.mesh.num_nodes, prob.mesh.num_elements
    got = {name: np.load(out / f"{name}.npy") for name in ("u", "f", "stress")}
    assert sorted(os.listdir(out)) == ["f.npy", "stress.npy", "u.npy"]
    assert got["u"].shape == got["f"].shape == (2 * N,) and got["stress"].shape == (E,)
    assert all(a.dtype == np.float64 and np.all(np.isfinite(a)) for a in got.values())
    known = prob.u_known == 1  # prescribed displacements come back as given, the free ones moved
    assert np.array_equal(got["u"][known], prob.u_in[known]) and np.abs(got["u"][~known]).max() > 0


@pytest.mark.parametrize("window", ["allreduce", "auto", "host-window"])
def test_bench_multi_rank_code_path_on_one_gpu(built, window):
    """bench.py as the driver launches it for N > 1 (torch.distributed.run, one process per rank), rehearsed with both
    ranks on the one GPU and gloo in place of RCCL (--share-gpu): stacked weak-scaling mesh, barriers, max-over-ranks
    timing, rank 0 prints the single line."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr",
           "127.0.0.1", "--master-port", str(29581 + len(window)), os.path.join(ROOT, "bench.py"), "--gpus", "2",
           "--share-gpu", "--workload", "plate100k", "--steps", "1", "--warmup", "1", "--full", "--op-reps", "20",
           "--exchange", window]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["scaling"] == "weak" and d["cpu_baseline"] is None and "rehearsal" in d
    assert d["config"]["parallelism"] == "hilbert-tile-ranges2" and d["config"]["ranks"] == 2 and d["config"]["elements"] == 2 * 100352
    assert d["cg_converged"] == 1 and d["value"] > 0 and d["verify"]["ok_on_every_rank"] is True
    if window == "host-window":  # two ranks x ~50 workgroups fit the one GPU side by side: the on-chip CG runs
        assert d["config"]["cg_kernel"] == 2 and "window" in d["config"]["exchange"]
    elif window == "allreduce":  # streaming kernels, one all-reduce per iteration
        assert d["config"]["cg_kernel"] == 1 and "all-reduce" in d["config"]["exchange"]
    else:                        # default: one untimed trial each way, the faster kept
        tune = d["config"]["exchange_autotune"]
        assert tune["kernel_with_inboxes"] == 2 and tune["s_per_solve_inboxes"] > 0 and tune["s_per_solve_allreduce"] > 0
        # the inbox path is only kept when it reproduced the all-reduce solve on every rank
        assert tune["solutions_agree_on_every_rank"] is True and tune["rel_l2_u_between_them"] <= 1e-8
        assert abs(tune["iterations_inboxes"] - tune["iterations_allreduce"]) <= 2
        faster = tune["s_per_solve_inboxes"] < tune["s_per_solve_allreduce"]
        assert d["config"]["cg_kernel"] == (2 if faster else 1)
        assert ("inboxes" in d["config"]["exchange"]) == faster


def test_bench_streaming_kernels_exchange_through_inboxes(built):
    """--cg-variant 1 --exchange inboxes: what a mesh too large for the chips gets (BASELINE config 5 on 8 GPUs) -- the
    streaming kernels trade through the device inboxes (k_stream_exchange, exchange_kind 3), kept only because the trial
    solve reproduced the all-reduce solve on both ranks."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr",
           "127.0.0.1", "--master-port", "29613", os.path.join(ROOT, "bench.py"), "--gpus", "2", "--share-gpu",
           "--workload", "plate100k", "--steps", "1", "--warmup", "1", "--full", "--op-reps", "20", "--cg-variant", "1",
           "--exchange", "inboxes"]
    r = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"), capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0])
    tune = d["config"]["exchange_autotune"]
    assert tune["exchange_with_inboxes"] == 3 and tune["solutions_agree_on_every_rank"] is True
    assert d["config"]["exchange_kind"] == 3 and d["config"]["cg_kernel"] == 1 and "k_stream_exchange" in d["config"]["exchange"]
    assert d["cg_converged"] == 1 and d["verify"]["ok_on_every_rank"] is True


def test_bench_strong_partition_keeps_the_baseline_size(built):
    """--partition strong: the workload at its BASELINE size split over the ranks (configs 4 and 5 are `--gpus 4
    --workload plate4m --partition strong` and `--gpus 8 --workload multihole16m --partition strong`); rehearsed with
    two ranks on the one GPU."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr",
           "127.0.0.1", "--master-port", "29611", os.path.join(ROOT, "bench.py"), "--gpus", "2", "--share-gpu",
           "--workload", "plate100k", "--steps", "1", "--warmup", "1", "--full", "--op-reps", "20", "--exchange", "allreduce",
           "--partition", "strong"]
    r = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"), capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0])
    assert d["n_gpus"] == 2 and d["scaling"] == "strong" and d["config"]["elements"] == 100352
    assert d["config"]["partition"] == "strong" and d["config"]["ranks"] == 2 and d["cg_converged"] == 1
    # per-GPU kernel figures: each rank's launch covers its half of the tiles
    assert d["spmv"]["bytes_per_launch"] == 12.0 * 100352 / 2 + 50.0 * 50625 / 2


def test_bench_bare_multi_gpu_launch(built):
    """`python bench.py --gpus 2 ...` with NO launcher around it -- the form the driver records for N = 1 and would use
    for N > 1: the parent starts its two ranks itself (torch.distributed.run as a child, before any GPU call), rank 0's
    single line comes through and the exit code is the children's."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--share-gpu", "--workload",
                        "plate100k", "--steps", "1", "--warmup", "1", "--full", "--op-reps", "20"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["ranks"] == 2 and d["cg_converged"] == 1 and d["capped"] is False
    assert d["verify"]["ok_on_every_rank"] is True and "rehearsal" in d
    # the label says what carried the all-reduce (gloo through the host callback here, RCCL on a node)
    assert d["config"]["transport"] == "callback"
    assert "RCCL" not in d["config"]["exchange"] or "inboxes" in d["config"]["exchange"]
    assert "plate100k" in d["metric"] and "1M-tri" not in d["metric"]


@pytest.mark.parametrize("exchange", ["allreduce", "inboxes"])
def test_config4_four_ranks_at_baseline_size_against_the_oracle_fixture(built, exchange):
    """BASELINE config 4 as written: the 4M-triangle plate split over FOUR ranks (--partition strong), streaming kernels,
    per-iteration exchange by all-reduce and through the device inboxes (k_stream_exchange); every rank compares the
    solution it returns with the oracle's sampled solution (tests/golden/fullsize_plate4m.npz: 7943 iterations, u at
    4096 DOFs <= 1e-8, reactions and stress <= 1e-7).  Ranks share the one GPU; started bare."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--share-gpu", "--partition",
                        "strong", "--workload", "plate4m", "--cg-variant", "1", "--exchange", exchange, "--steps", "1",
                        "--warmup", "0", "--full", "--op-reps", "20", "--check-fixture"], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0])
    fp = d["fixture_parity"]
    assert fp["ok"] is True and fp["ok_on_every_rank"] is True, fp
    assert fp["iterations"] == fp["oracle_iterations"] == 7943 and fp["mesh_is_the_fixtures"] is True
    assert fp["rel_l2_u_sampled"] <= 1e-8 and fp["rel_l2_stress_sampled"] <= 1e-7
    assert d["n_gpus"] == 4 and d["scaling"] == "strong" and d["config"]["elements"] == 3998792
    assert d["config"]["exchange_kind"] == (3 if exchange == "inboxes" else 1) and d["config"]["cg_kernel"] == 1
    assert d["verify"]["ok_on_every_rank"] is True and d["capped"] is False


def test_on_chip_kernels_of_two_ranks_with_four_tiles_per_workgroup_against_the_oracle_fixture(built):
    """The multi-GPU on-chip kernel at the load it has on a node -- four 512-node tiles per workgroup, sibling tiles reading
    each other's LDS slots, the live halo entries compacted, nodes only siblings read publishing nothing locally -- which the
    8-rank rehearsals (one tile per workgroup) never reach: the 1M-triangle mesh of BASELINE config 3 split over TWO ranks that
    share the one GPU (MAG_TUNE_PERSIST_K=4 makes each rank's grid 123 workgroups, so both launches are co-resident),
    device inboxes, every rank against the oracle's sampled solution (5389 iterations, u <= 1e-8)."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["MAG_TUNE_PERSIST_K"] = "4"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--share-gpu", "--partition",
                        "strong", "--workload", "hole1m", "--exchange", "inboxes", "--steps", "1", "--warmup", "1",
                        "--full", "--op-reps", "20", "--no-cpu-baseline", "--no-hbm-resident", "--check-fixture"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0])
    fp = d["fixture_parity"]
    assert fp["ok"] is True and fp["ok_on_every_rank"] is True, fp
    assert fp["iterations"] == fp["oracle_iterations"] == 5389 and fp["rel_l2_u_sampled"] <= 1e-8
    assert d["config"]["cg_kernel"] == 2 and d["config"]["exchange_kind"] == 2 and d["fallback"] is False
    assert d["verify"]["ok_on_every_rank"] is True and d["capped"] is False


def test_bench_refuses_to_pass_a_capped_solve_for_a_result(built):
    """mag_run returns MAG_OK at the iteration cap (solver.rs:149-176 returns Ok(best_param)); a bench line measured on
    such steps is marked and the process exits non-zero"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "plate100k", "--steps", "1",
                        "--warmup", "0", "--max-iter", "300", "--no-cpu-baseline", "--no-hbm-resident", "--op-reps", "20"],
                       cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 5, r.stdout[-2000:] + r.stderr[-2000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0])
    assert d["capped"] is True and d["cg_converged"] == 0 and d["cg_termination"] == "max_iters"
    assert d["cg_iterations"] == 300 and 0 < d["cg_best_iteration"] <= 300
    assert "not a result" in r.stderr


def test_smoke_entry_point(built):
    r = subprocess.run([sys.executable, "-c", "import __graft_entry__ as g; g.smoke()"], cwd=ROOT, capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


def test_two_processes_share_the_gpu(built):
    """Two processes solve the benchmark mesh at the same time, each with the on-chip CG as its default.  That kernel
    needs every workgroup resident; when the other process holds part of the GPU its grid-wide waits give up within
    their spin budget and the solve is redone by the streaming kernels -- slower, never wrong, never hung."""
    worker = os.path.join(ROOT, "tests", "concurrent_worker.py")
    procs = [subprocess.Popen([sys.executable, worker, "4"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                              text=True) for _ in range(2)]
    results = []
    for pr in procs:
        so, se = pr.communicate(timeout=600)
        assert pr.returncode == 0, so[-2000:] + se[-2000:]
        results.append(json.loads([l for l in so.splitlines() if l.startswith("[")][-1]))
    runs = [r for res in results for r in res]
    assert all(r["converged"] == 1 and abs(r["iterations"] - 5389) <= 2 for r in runs), runs
    # the same kernel gives the same bits in either process; the two kernels agree to rounding (checked elsewhere)
    for kernel in (1, 2):
        assert len({r["digest"] for r in runs if r["kernel"] == kernel}) <= 1, runs
