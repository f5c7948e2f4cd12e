"""Helpers of tests/test_dist_krylov.py: one rank of a sharded MG-preconditioned Krylov solve on the halo form
(multigrid.jl_amd/distributed.py: DistributedHierarchy = the Python sequencer, NativeDistributedHierarchy = mg_dist_*), the
parent that gathers the ranks' results, and the oracle they are held against."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from test_distributed import _free_port, _problem  # noqa: E402  (the problems of the sharded-cycle tests)

TOL = 1e-9
INNER = 3


def max_iter(kind):
    return 40 if kind == "sa" else 12


def start_vector(method, n):
    """BiCGSTAB starts from a seeded non-zero x0 (the initial-residual product needs x's halo), the others from zero."""
    if method == "bicgstab":
        return 0.01 * np.random.default_rng(3).standard_normal(n)
    return np.zeros(n)


def oracle_solve(kind, cyc, method):
    from oracle import mg_oracle as orc
    _, A, p, b, _ = _problem(kind, 1, cyc)
    p.relativeTol, p.maxOuterIter = TOL, max_iter(kind)
    x0 = start_vector(method, A.shape[0])
    if method == "pcg":
        x, flag, it, resvec = orc.solveCG_MG(p, b, x0)
    elif method == "bicgstab":
        x, flag, it, resvec = orc.solveBiCGSTAB_MG(p, b, x0)
    else:
        x, flag, it, resvec = orc.solveGMRES_MG(p, b, x0, INNER)
    return x, int(flag), int(it), np.asarray(resvec)


def worker(rank, world, port, kind, cyc, method, mode, box, q):
    """mode: "cpu" (gloo, Python sequencer, CpuCheckerBackend), "plugin" (native sequencer, ranks share cuda:0, host-staged
    transport over gloo), "rccl" (native sequencer, RCCL transport)."""
    try:
        use_hip = mode != "cpu"
        if box and use_hip:       # let the small local operators of the test take the row-class / staged kernels
            os.environ.update(MG_NO_SMALL="1", MG_ROWCLASS_MIN_ROWS="0", MG_ROWCLASS_MAX_PASSES="64", MG_ROWCLASS_MIN_COVER="0.3",
                              MG_MARCH_MIN_WG="0", MG_TILE_MIN_WG="0", MG_WINDOW_MIN_WG="0", MG_MARCH_MAX_LEN="64",
                              MG_WINP_MIN_ROWS="0")
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        if mode == "rccl":
            torch.cuda.set_device(0)
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", 0))
        else:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        from multigrid_jl_amd import distributed as dd
        _, A, p, b, nodes = _problem(kind, 1, cyc)
        owner = dd.box_owner(nodes, dd.default_domains(world, len(nodes))) if nodes is not None else dd.block_owner(A.shape[0], world)
        if use_hip:
            be, comm = dd.HipBackend(0), dd.TorchComm(stage_through_host=(mode != "rccl"))
        else:
            from dist_cpu_backend import CpuCheckerBackend
            be, comm = CpuCheckerBackend(), dd.TorchComm()
        level_nodes = None
        if box and nodes is not None:
            level_nodes = [((np.asarray(nodes) - 1) >> l) + 1 for l in range(len(p.As))]
        H = dd.DistributedHierarchy.from_global(p, comm, be, owner, 1, replicate_below=200, level_nodes=level_nodes)
        assert len(H.levels) >= 2, "the test must exercise at least two sharded levels"
        assert H.box_form == bool(box and nodes is not None)
        S = dd.NativeDistributedHierarchy(H, transport=mode) if use_hip else H
        b_loc = H.scatter_fine(b)
        # what ONE application of the preconditioner communicates (a cycle from x = 0)
        e0, a0 = S.comm_stats()
        S.cycle(b_loc, torch.zeros_like(b_loc), True)
        e1, a1 = S.comm_stats()
        x_loc = H.scatter_fine(start_vector(method, A.shape[0]))
        maxit = max_iter(kind)
        if method == "pcg":
            flag, it, resvec = S.pcg(b_loc, x_loc, TOL, maxit)
        elif method == "bicgstab":
            flag, it, resvec = S.bicgstab(b_loc, x_loc, TOL, maxit)
        else:
            flag, it, resvec = S.fgmres(b_loc, x_loc, INNER, TOL, maxit)
        e2, a2 = S.comm_stats()
        be.synchronize()
        info = dict(e_cyc=e1 - e0, a_cyc=a1 - a0, exchanges=e2 - e1, allreduces=a2 - a1)
        out = [None] * world
        dist.all_gather_object(out, (H.rows_fine, x_loc.cpu().numpy(), int(flag), int(it), np.asarray(resvec), info))
        if rank == 0:
            x = np.zeros_like(b)
            for rows, xl, *_ in out:
                x[rows] = xl
            q.put(("ok", [o[2] for o in out], [o[3] for o in out], [o[4] for o in out], x, [o[5] for o in out]))
        dist.barrier()
        if use_hip:
            S.close()
        dist.destroy_process_group()
    except Exception as e:  # pragma: no cover
        import traceback
        q.put(("err", f"rank {rank}: {e!r}\n{traceback.format_exc()}"))


def run(world, kind, cyc, method, mode, box=False):
    """Run the ranks, compare with the oracle (flag, count, resvec and x to 1e-10), return (iterations, per-rank comm info)."""
    x_ref, flag_ref, it_ref, res_ref = oracle_solve(kind, cyc, method)
    maxit = max_iter(kind)
    # the case must compare a converged solve, not the cap: flag 0 in the oracle after more than one iteration, before maxIter
    assert flag_ref == 0 and it_ref > 1, (flag_ref, it_ref)
    assert it_ref < (INNER * maxit if method == "fgmres" else maxit), it_ref
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=worker, args=(r, world, port, kind, cyc, method, mode, box, q)) for r in range(world)]
    for pr in procs:
        pr.start()
    try:
        res = q.get(timeout=300)
    finally:
        for pr in procs:
            pr.join(timeout=60)
            if pr.is_alive():
                pr.kill()
    assert res[0] == "ok", res[1]
    _, flags, its, resvecs, x, infos = res
    print(f"{kind}/{cyc}/{method}/{mode} world {world}: flag {flags} iters {its} (oracle {flag_ref}, {it_ref}), comm {infos[0]}")
    assert all(f == flag_ref for f in flags) and all(i == it_ref for i in its), (flags, flag_ref, its, it_ref)
    for rv in resvecs:                      # every rank holds the same, global, residual history
        assert len(rv) == len(res_ref), (len(rv), len(res_ref))
        print("  max |resvec - oracle| =", np.abs(rv - res_ref).max())
        assert np.abs(rv - res_ref).max() <= 1e-10 * max(1.0, np.abs(res_ref).max()), (rv, res_ref)
    print("  max |x - oracle| / max |oracle| =", np.abs(x - x_ref).max() / np.abs(x_ref).max())
    assert np.abs(x - x_ref).max() <= 1e-10 * np.abs(x_ref).max()
    return it_ref, infos


def check_communication(method, k, infos):
    """The communication outside the preconditioner is what the drivers were designed to issue (k: the oracle's count)."""
    for i in infos:
        ec, ac = i["e_cyc"], i["a_cyc"]
        assert ec > 0
        if method == "pcg":         # k iterations, the k-th converged: products 1 + k, cycles k; scalars ||b||, (r'z, r'r), then 2 per iteration
            cycles, products, scalars = k, 1 + k, 2 + 2 * k
        elif method == "bicgstab":  # per iteration 2 cycles, 2 products, 3 all-reduces; ||b||, ||r0|| in front
            cycles, products, scalars = 2 * k, 1 + 2 * k, 2 + 3 * k
        else:                       # k inner steps in R restarts: a cycle and a product per step + a residual per restart; 2 all-reduces per step
            restarts = -(-k // INNER)
            cycles, products, scalars = k, 1 + k + (restarts - 1), 2 + 2 * k + (restarts - 1)
        assert i["exchanges"] - cycles * ec == products, (i, k)       # level-1 exchanges outside the cycle: one per product with A
        assert i["allreduces"] - cycles * ac <= scalars, (i, k)
