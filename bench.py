"""Benchmark: particle-steps/s (B*N*T / s) of DPF.filtering_pos on synthetic disk tracking.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--config c2] [--dump-outputs DIR] [--full]

A plain run sets up, warms up, times the K steps and prints the result line (value, ms_per_step,
the last pass's RMSE and resampled steps).  --full adds what takes runs of its own after them: the
live roofline of the dominant launch, the resampler on its own, the RMSE on informative
encodings, the `forced` and `informative` lines and the CPU baseline ([--no-cpu-baseline]
[--no-forced] [--no-informative] leave one out).  --dump-outputs DIR writes the last timed pass's
outputs as DIR/<name>.npy (dump_outputs).

A "step" is one filtering_pos pass over one batch (B, N, T) -- the hot path of
BASELINE.json, with the frame encoder replaced by precomputed encodings exactly as the
reference CPU path was timed.  Default workload = BASELINE configs[1]
(C2: CNF-DPF, --NF-dyn --NF-cond, RealNVP, cos measurement, soft resampling, N=1000, B=64,
T=50), device-RNG mode, ESS-gated as the reference.

Multi-GPU (torch.distributed.run, one process per GPU, RCCL): weak scaling, B rows per rank;
the only per-step exchange is an all-gather of the B per-row ESS terms so the batch-global
resampling gate of DPFs.py:163-165 is taken identically on every rank.
"""
import argparse
import json
import os
import platform
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.join(ROOT, "normalizing-flows-dpfs_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

CONFIGS = {
    # name: (flags, B, N, T, algorithmic FLOP per particle-step,
    #        of which in the proposal+measurement launch of the tiled pipeline)
    # (EXECUTED FLOP of that launch, where it differs, are in F_EXEC below)
    # C2 matmul FLOP per particle: nf_dyn inverse 1,792 + proposal 5,888 +
    # nf_dyn forward 1,792 + cos measurement 3,136 = 12,608, x 13.1/12.608 elementwise.
    "c1": (dict(NF_dyn=False, NF_cond=False, measurement="cos", resampler_type="soft"), 16, 100, 24, 3.3e3, 3.3e3),
    "c2": (dict(NF_dyn=True, NF_cond=True, measurement="cos", resampler_type="soft"), 64, 1000, 50, 13.1e3,
           13.1e3 * (5888 + 1792 + 3136) / 12608),
    "c3": (dict(NF_dyn=False, NF_cond=False, measurement="CRNVP", resampler_type="ot"), 64, 1000, 50, 12.7e3,
           12.7e3),
    # C4: B=256 over 8 GPUs -> 32 rows per GPU; MAF dynamic flow, OT (9.8k + OT)
    "c4": (dict(NF_dyn=True, NF_cond=True, measurement="cos", resampler_type="ot", NF_dyn_flow="MAF"), 32, 4000,
           50, 9.8e3, 9.8e3),
    # C5: B=512 over 8 GPUs -> 64 rows per GPU, N=10000, T=100, CGLOW measurement (--hiddensize 192);
    # 201k FLOP per particle-step, of which the CGLOW kernel (A13) 13,376 + 158,080
    "c5": (dict(NF_dyn=True, NF_cond=True, measurement="CGLOW", resampler_type="soft", hiddensize=192), 64,
           10000, 100, 201e3, 13376 + 158080),
}
# FLOP per particle the proposal launch actually executes: the per-row context columns of the
# coupling nets' first layers (36 of 37 inputs of the proposal's, 4 of 5 of nf_dyn's) are
# folded into per-row biases once per row, so a coupling net runs 1->8->8->1:
# (8 + 64 + 8) MAC x 2 FLOP x 2 nets x 2 halves x 2 flows = 1,280 per stack.
# C2: proposal inverse 1,280 + nf_dyn forward 1,280 + cosine encoder 3,136 = 5,696.
# C4: proposal 1,280 + MAF forward 2 x 176 + cosine encoder 3,136 = 4,768.
F_EXEC = {"c2": 5696.0, "c4": 4768.0}
# ... of the whole step when it runs as one launch (tiled_step_fused_kernel): + the nf_dyn
# inverse's executed 1,280 (4 coupling halves x 2 nets x (1 + 8x8 + 8) MAC; 4 of its 5 inputs are
# the per-row context, folded)
F_EXEC_STEP = {"c2": 6976.0}
# the merged front launch (tiled_fdyn_kernel): the nf_dyn inverse, 1,792 matmul FLOP (A9) scaled
# by 13.1 / 12.608 for the elementwise work; executed 1,280 (its [mean, std] context folded)
F_DYN_INV = 1792.0 * 13.1 / 12.608
F_DYN_INV_EXEC = 1280.0
B_ALG = 52.0            # algorithmic HBM bytes per particle-step
B_SOFT = 36.0           # soft resampling, HBM bytes per particle: read x 8 + p 4,
#                         write x' 8 + w' 4 + index 8, + 4 for the row's CDF pass
PEAK_FP32_TFLOPS = 157.3  # MI355X_MICROARCH.md: FP32 vector = FP32 MFMA dense peak
PEAK_HBM_GBS = 8000.0


def make_args(flags, B, N, T, extra):
    from arguments import parse_args
    a = parse_args([])
    a.num_particles, a.batchsize, a.sequence_length = N, B, T
    for k, v in {**flags, **extra}.items():
        setattr(a, k, v)
    return a


def synthetic_disk(B, T, seed, E):
    """Disk trajectories from the reference's process model (create_dataset.py:197-216):
    spring 0.1, drag 0.0075, position noise 2.0, init pos U[-64,64]^2, vel N(0,1)*3; the
    control input is the true velocity + N(0, 4^2) (DPFs.py:105); frame encodings N(0,1)."""
    g = np.random.default_rng(seed)
    pos = g.uniform(-64, 64, size=(B, 2))
    vel = g.normal(size=(B, 2)) * 3
    start = np.concatenate([pos, vel], -1)
    states = []
    for _ in range(T):
        pull, drag = -0.1 * pos, -0.0075 * vel ** 2 * np.sign(vel)
        pos = pos + vel + g.normal(scale=2.0, size=(B, 2))
        vel = vel + pull + drag
        states.append(np.concatenate([pos, vel], -1))
    state = np.stack(states, 1).astype(np.float32)
    vel_in = state[:, :, 2:] + g.normal(scale=4.0, size=(B, T, 2)).astype(np.float32)
    enc = g.normal(size=(B, T, E)).astype(np.float32)
    return (torch.from_numpy(start.astype(np.float32)), torch.from_numpy(state), torch.from_numpy(vel_in),
            torch.from_numpy(enc))


def cgroup_cpus():
    """CPUs this process's cgroup may use (cgroup v2 cpu.max / v1 cfs quota), None if unlimited."""
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            return max(1, -(-int(q) // int(per)))
    except (OSError, ValueError):
        pass
    try:
        q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
        per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
        if q > 0:
            return max(1, -(-q // per))
    except (OSError, ValueError):
        pass
    return None


def cpu_threads():
    """The CPU baseline's thread count: NFDPF_CPU_THREADS if set, else every CPU of the process's
    affinity mask that its cgroup quota lets run at once (on the GPU box the mask lists the whole
    machine while the quota is the box's share: threads beyond the quota only time-slice)."""
    env = os.environ.get("NFDPF_CPU_THREADS")
    if env:
        return int(env)
    n = len(os.sched_getaffinity(0))
    q = cgroup_cpus()
    return min(n, q) if q else n


def cpu_baseline(cfg_name, seconds_budget=25.0, force=False):
    """The oracle (PyTorch-CPU restatement, timing-faithful: O(N^2) marker matching, FP64
    Sinkhorn, torch.cat history) on the host cores, on a bounded sample of the workload."""
    from oracle import dpf_oracle as O
    flags, B, N, T, _, _ = CONFIGS[cfg_name]
    cores = cpu_threads()
    torch.set_num_threads(cores)
    torch.manual_seed(2)
    a = make_args(flags, B, N, T, {})
    from DPFs import DPF
    dpf = DPF(a)
    params = {k: v.detach().float().cpu() for k, v in dpf.state_dict().items()}
    start, state, vel, enc = synthetic_disk(B, T, 2, a.hiddensize)
    Bs, Ts = B, T
    if flags["resampler_type"] == "ot":
        Bs, Ts = max(1, B // 16), min(T, 10)   # one FP64 OT call is tens of seconds at B=64
        if force:
            Bs, Ts = max(1, B // 16), 4        # every step calls the FP64 Sinkhorn
    if N >= 4000:
        Bs, Ts = 4, 8                          # C5: 4 rows x 8 steps (dense N^2 resampler work)
        if flags["resampler_type"] == "ot":
            # C4: one row; the ESS gate first fires after ~12 steps, so 16 steps hold a few
            # FP64 Sinkhorn calls (~10 s each at N=4000) -- 8 rows x 8 steps would hold none
            Bs, Ts = 1, 16
    cfg = dict(N=N, NF_dyn=flags["NF_dyn"], NF_cond=flags["NF_cond"], measurement=flags["measurement"],
               resampler=flags["resampler_type"], alpha=0.5, eps=0.1, scaling=0.75, threshold=1e-3, max_iter=100,
               pos_noise=20.0, vel_noise=20.0, width=128, n_flows=2, cglow_K=1,
               dyn_flow=flags.get("NF_dyn_flow", "RealNVP"))
    ot_calls = []
    ot_orig = O.ot_resample

    def ot_counted(*a, **k):
        ot_calls.append(1)
        return ot_orig(*a, **k)

    O.ot_resample = ot_counted
    run = lambda: O.filtering(cfg, params, enc[:Bs, :Ts], start[:Bs], vel[:Bs, :Ts], rng=O.HostRNG(),  # noqa: E731
                              force_resample=force)
    with torch.no_grad():
        t0 = time.perf_counter()
        run()  # warm-up
        one = time.perf_counter() - t0
        reps = max(1, min(3, int(seconds_budget / max(one, 1e-3)) - 1))
        times = []
        for _ in range(reps):
            t0 = time.perf_counter()
            run()
            times.append(time.perf_counter() - t0)
    O.ot_resample = ot_orig
    med = float(np.median(times))
    ot_note = ""
    if flags["resampler_type"] == "ot":
        ot_note = f", OT resampling in {len(ot_calls) // (reps + 1)} of {Ts} steps"
    q = cgroup_cpus()
    return {"value": Bs * N * Ts / med, "unit": "particle-steps/s", "cores": cores, "kind": "port",
            "cpu_affinity": len(os.sched_getaffinity(0)), "cgroup_cpus": q,
            "sample": f"oracle filtering B={Bs} N={N} T={Ts} ({'forced' if force else 'ESS-gated'} resampling"
                      f"{ot_note}), median of {reps} after 1 "
                      f"warm-up; host {platform.processor() or platform.machine()}"}


# Sinkhorn iteration (resamplers.py:131-153): per particle pair (i, j) of a row, the cost
# |x~_i - x~_j|^2 / 2 (4 FLOP) and the two live softmins' f_j - C_ij / eps, max-shift, exp,
# sum (5 each, the exp counted as one) -- the reference's algorithm, a_x / b_y excluded
F_OT_PAIR = 14.0


def ot_iteration_ms(res, T):
    """Average duration of one Sinkhorn iteration launch (ot_iter_kernel) on this workload's
    particles (history slot T/2): two stream-ordered OT calls forced to 10 and 20 iterations
    (stop_at), hipEvents around each; the difference / 10 leaves the fixed launches out."""
    from nfdpf import ops
    x = res.particles[:, T // 2].contiguous()
    w = res.probs[:, T // 2].contiguous()
    out = {}
    for k in (10, 20):
        stop = torch.full((1,), k + 2, dtype=torch.int32, device=x.device)
        best = None
        for _ in range(3):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            ops.ot_resample(x, w, stop_at=stop, poll=False)
            b.record()
            torch.cuda.synchronize()
            best = a.elapsed_time(b) if best is None else min(best, a.elapsed_time(b))
        out[k] = best
    it = (out[20] - out[10]) / 10.0
    # ranks rehearsed on ONE shared GPU time each other's launches too; a difference the other
    # rank's work swamped falls back to the 20-iteration call's share, which includes the
    # per-call fixed passes (an upper bound: flagged in the record, and no roofline from it)
    if it > 0:
        return it, False
    return out[20] / 20.0, True


def soft_resample_ms(res, T, reps=20):
    """Average duration of the standalone soft resampler (nfdpf_soft_resample ->
    soft_resample_kernel, resamplers.py:20-60) on this workload's particles (history slot T/2):
    one event pair around ``reps`` back-to-back calls after a warm-up."""
    from nfdpf import ops
    x = res.particles[:, T // 2].contiguous()
    p = res.probs[:, T // 2].contiguous()
    off = torch.rand(p.shape[0], device=p.device) / p.shape[1]
    ops.soft_resample(x, p, 0.5, off)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        ops.soft_resample(x, p, 0.5, off)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def ot_call_ms(res, T, iters=10):
    """Whole OT resampler call (all launches) forced to ``iters`` iterations, best of 3."""
    from nfdpf import ops
    x = res.particles[:, T // 2].contiguous()
    w = res.probs[:, T // 2].contiguous()
    stop = torch.full((1,), iters + 2, dtype=torch.int32, device=x.device)
    best = None
    for _ in range(3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        ops.ot_resample(x, w, stop_at=stop, poll=False)
        b.record()
        torch.cuda.synchronize()
        best = a.elapsed_time(b) if best is None else min(best, a.elapsed_time(b))
    return best


def rocprof_avg_ms(tag, kname, instance=None):
    """Average duration (ms) of ``kname`` in the committed rocprofv3 --kernel-trace --stats
    summary of this workload's bench command (scripts/r06.sh prof -> profiles/rocprof_<tag>.csv,
    tag = config [+ _force]), and the file; (None, None) when there is none.  ``instance``: the
    template instance's name prefix (e.g. "tiled_pass_kernel<0,": the speculative pass) -- the
    summary of one bench command holds its forced and informative lines' instances too."""
    path = os.path.join(ROOT, "profiles", f"rocprof_{tag}.csv")
    if not os.path.exists(path):
        return None, None
    import csv
    rows = list(csv.DictReader(open(path)))
    if instance is not None:
        for row in rows:
            if row["Name"].split("::", 1)[-1].startswith(instance):
                return float(row["AverageNs"]) * 1e-6, os.path.relpath(path, ROOT)
    # "<kernel>[full]" (scripts/rocprof_ot_split.py): the Sinkhorn launches that ran an iteration,
    # without the early-exit tail the plain row averages in
    for want in (kname + "[full]", kname):
        for row in rows:
            full = row["Name"].endswith("[full]")
            name = row["Name"].split("(")[0].split("::")[-1].split("<")[0].strip() + ("[full]" if full else "")
            if name == want and (full == want.endswith("[full]")):
                return float(row["AverageNs"]) * 1e-6, os.path.relpath(path, ROOT)
    return None, None


def pmc_traffic(cfg_name, kname):
    """HBM bytes per launch of ``kname`` from the committed PMC summary of this workload
    (scripts/pmc.sh + scripts/pmc_summary.py -> profiles/pmc_<tag>.csv, tag = config [+ _force]):
    FETCH_SIZE and WRITE_SIZE are KiB; gfx950 FETCH_SIZE counts half the bytes of a streaming
    read (MI355X_MICROARCH.md, HBM / rocprofv3), so it is doubled.  None when no summary exists."""
    path = os.path.join(ROOT, "profiles", f"pmc_{cfg_name}.csv")
    if not os.path.exists(path):
        return None, None
    vals = {}
    for line in open(path).read().splitlines()[1:]:
        k, c, _, v = line.split(",")
        if k.split("::")[-1] == kname:
            vals[c] = float(v)
    if "FETCH_SIZE" not in vals or "WRITE_SIZE" not in vals:
        return None, None
    return (2.0 * vals["FETCH_SIZE"] + vals["WRITE_SIZE"]) * 1024.0, os.path.relpath(path, ROOT)


def trained_like(dpf, state, seed=1000):
    """A copy of the DPF with trained-like CRNVP-measurement weights (the C3 full-size parity
    case's model, tests/_fullsize.py c3_full: particle encoder ~ N(0, 0.5^2), conditional-RealNVP
    flows ~ N(0, 0.1^2), seeded) and its informative frame encodings (its particle encoder at the
    true positions + 30 % noise): the likelihood is sharp, the ESS gate fires on most steps and the
    OT resampler runs there -- the regime of a trained DPF-CM, which the reference init (flows
    ~ N(0, 0.01^2): an almost flat likelihood) never reaches."""
    import copy
    m = copy.deepcopy(dpf)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for mod, std in ((m.particle_encoder, 0.5), (m.cnf_measurement.flows, 0.1)):
            for p in mod.parameters():
                p.copy_((torch.randn(p.shape, generator=g) * std).to(p.device))
        enc = m.particle_encoder(state[:, :, :2].float())
        noise = torch.randn(enc.shape, generator=g).to(enc.device)
        enc = (enc + 0.3 * enc.abs().mean() * noise).contiguous()
    return m, enc


def timed_passes(fcfg, dpf, enc, start, vel_in, shard, args, world, dev):
    """W warm-up passes, then K passes timed between barriers + synchronisations (hipGraph
    replay of the whole pass where the pass has no host synchronisation), then (--full) one
    more Python-launched pass carrying the live kernel events.  -> dict."""
    from nfdpf.engine import FilterEngine
    eng = FilterEngine(fcfg, dpf)

    def step():
        return eng.run(enc, start, vel_in, shard=shard)

    for _ in range(max(1, args.warmup)):
        res = step()
    torch.cuda.synchronize()
    graph = None
    # auto (engine.FilterEngine.run): speculative gates when sharded, for OT at any world size
    # unless the previous pass resampled, and wherever the whole pass runs as one launch
    # the engine's own decision for the next pass (engine._decide_spec); a pass following a gate
    # plan (engine._plan_select) is verified after it the same way
    spec = eng.speculates(shard) or eng.plans(shard)
    # one GPU, a gated or forced one-launch pass (gates decided inside the launch): captured with
    # finish=False too, so that each replay's fault flags are checked (finish_pending) -- a replay
    # whose row hand-offs timed out is rerun, never taken for a result
    decided = world == 1 and eng.last_pass and not spec
    if args.graph and ((fcfg.resampler == "soft" and world == 1) or spec):
        # the pass has no host synchronisation in this mode: capture it once, replay per step
        # (every launch of every time step runs on each replay; only the Python launch path goes).
        # Speculative gate: the pass (engine.run(finish=False): no exchange inside) is captured;
        # after each replay finish_pending() gathers all steps' partials once (sharded),
        # verifies the T gates and reduces the obs-likelihood -- a fired gate (never at the
        # bench's init weights) reruns the pass step by step, inside the timing.
        # One GPU, speculative: TWO graphs (two sets of pass outputs) replayed alternately, and
        # pass k's verification -- its epilogue's flags, copied to pinned host memory right after
        # the replay -- read once an event behind that copy completes, while pass k + 1 already
        # runs: the host round trip no longer leaves the GPU idle between passes.  A fired gate
        # reruns pass k (gated) before the next replay; the last pass is verified inside the
        # timing.
        # (sharded, round 6: the same, the verification's small all-gather and gate kernels staged
        # on the stream behind each replay and its result copied to pinned host memory)
        pipelined = spec or decided
        graphs, caps, pends = [], [], []
        try:
            for _ in range(2 if pipelined else 1):
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    res = eng.run(enc, start, vel_in, shard=shard, finish=not (spec or decided))
                graphs.append(g)
                caps.append(res)
                pends.append(eng.take_pending() if (spec or decided) else None)
            for g in graphs:
                g.replay()
            torch.cuda.synchronize()
            graph = graphs[0]
        except RuntimeError as e:  # capture refused: keep the Python launch path
            print(f"bench: hipGraph capture failed ({e}); timing Python launches", file=sys.stderr)
            graph = None
            torch.cuda.synchronize()

        def step_graph():
            graph.replay()
            if pends[0] is not None and not eng.finish_pending(pends[0]):
                return eng.run(enc, start, vel_in, shard=shard, speculate=False)
            return caps[0]

        evs_done = [torch.cuda.Event(), torch.cuda.Event()]
        pipe = {"k": 0, "prev": None}

        def verify_prev():
            j = pipe["prev"]
            if j is None:
                return None
            pipe["prev"] = None
            if not eng.wait_flags(pends[j]):  # (flags not host-mapped: an event behind the copy)
                evs_done[j].synchronize()
            if not eng.finish_pending(pends[j], synced=True):
                return eng.run(enc, start, vel_in, shard=shard, speculate=False)
            return caps[j]

        def step_pipe():
            i = pipe["k"] & 1
            eng.arm_flags(pends[i])
            graphs[i].replay()
            if world > 1 or (pends[i][6] is not None and pends[i][6][0] is not None):
                eng.stage_flags(pends[i])  # flags on the device (or sharded: the gather): stage a copy
                evs_done[i].record()
            out = verify_prev()
            pipe["prev"], pipe["k"] = i, pipe["k"] + 1
            return out if out is not None else caps[i]
        step_pipe.drain = verify_prev
        if graph is not None:
            step = step_pipe if pipelined else step_graph  # noqa: F811
    elif spec and world == 1 and eng.last_pass:
        # --graph 0, one GPU, a speculative one-launch pass: the same pipelining with Python
        # launches -- pass k + 1 is launched (run(finish=False)) before pass k's flags are waited
        # for, so the host's launch path overlaps the GPU (fresh outputs per pass)
        pp = {"prev": None}

        def verify_prev_py():
            prev = pp["prev"]
            if prev is None:
                return None
            pp["prev"] = None
            pend, out = prev
            if not eng.wait_flags(pend):
                torch.cuda.current_stream().synchronize()
            if not eng.finish_pending(pend, synced=True):
                return eng.run(enc, start, vel_in, shard=shard, speculate=False)
            return out

        def step_py_pipe():
            out = eng.run(enc, start, vel_in, shard=shard, finish=False)
            pend = eng.take_pending()
            done = verify_prev_py()
            pp["prev"] = (pend, out)
            return done if done is not None else out
        step_py_pipe.drain = verify_prev_py
        step = step_py_pipe  # noqa: F811
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    eng.step_events = None  # the timed passes carry no events (host cost of creating them)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        res = step()
    if getattr(step, "drain", None) is not None:  # the last pipelined pass's verification
        res = step.drain() or res
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if world > 1:
        tt = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt.item())
    if not args.full:  # a plain run: the headline figure alone, no live kernel timing
        return dict(res=res, elapsed=elapsed, kernel_ms=None, front_ms=None, eng=eng, graph=graph, spec=spec)
    # live kernel timing: one more pass right after the timed ones, Python-launched (event nodes
    # inside a graph cannot be timed on ROCm 7), identical kernels and inputs; the tiled step's
    # events ride in the timed launch's own dispatch (hipExtLaunchKernel), every step
    eng.step_events = []
    eng.run(enc, start, vel_in, shard=shard)
    torch.cuda.synchronize()
    evs = eng.step_events
    eng.step_events = None
    kernel_ms = float(np.mean([e.ms() for e in evs]))
    front = [e.ms(1) for e in evs if e.n == 4]
    front_ms = float(np.mean(front)) if front else None
    for e in evs:
        e.close()
    return dict(res=res, elapsed=elapsed, kernel_ms=kernel_ms, front_ms=front_ms, eng=eng, graph=graph, spec=spec)


DUMP_BYTES = 48 << 20   # --dump-outputs: all files together stay below this (the arrays' data)


def dump_outputs(res, out_dir):
    """Write the last timed pass's FilterResult -- what a caller of FilterEngine.run receives:
    particles, probs, noise, lik, init_logw, index, jac, prior, obs_likelihood, pred (those that
    are not None) -- as ``out_dir/<name>.npy``, float32 (integer tensors: float64, exact).  The
    inputs, the model and the device RNG are seeded, so two runs with the same arguments write the
    same arrays.  An array beyond its share of DUMP_BYTES is written as a fixed sample: its
    flattened elements at sorted indices drawn from a generator seeded with 0 (the same indices
    for the same shape in every run)."""
    os.makedirs(out_dir, exist_ok=True)
    names = ("particles", "probs", "noise", "lik", "init_logw", "index", "jac", "prior", "obs_likelihood", "pred")
    arrs = {}
    for name in names:
        t = getattr(res, name, None)
        if torch.is_tensor(t):
            t = t.detach()
            arrs[name] = t.double() if not t.is_floating_point() else t.float() if t.dtype != torch.float64 else t
    share = DUMP_BYTES // max(1, len(arrs))
    for name, t in arrs.items():
        keep = share // t.element_size()
        if t.numel() > keep:
            idx = np.sort(np.random.default_rng(0).integers(0, t.numel(), size=keep))
            t = t.reshape(-1)[torch.from_numpy(idx).to(t.device)]
        np.save(os.path.join(out_dir, name + ".npy"), t.cpu().numpy())


def dominant(cfg_name, flags, kernel, B, N, T, fcfg, run, force):
    """The pass's dominant launch and its algorithmic cost per unit, timed
    live (run['kernel_ms'] / run['front_ms']) or, for the Sinkhorn, by ot_iteration_ms."""
    _, _, _, _, F_STEP, F_PROP = CONFIGS[cfg_name]
    eng, kernel_ms, front_ms, res = run["eng"], run["kernel_ms"], run["front_ms"], run["res"]
    F_ALG = F_PROP if (kernel == "tiled" or flags["measurement"] == "CGLOW") else F_STEP
    units, nbytes = B * N, B_ALG * B * N  # per launch of the step kernels
    kname = "filter_step_kernel"
    if kernel == "tiled":  # the proposal launch (csrc/filter_tiled.hip launch_prop)
        if fcfg.split_nets and flags["NF_dyn"] and flags["NF_cond"] and flags["measurement"] == "cos" \
                and flags.get("NF_dyn_flow", "RealNVP") == "RealNVP":
            kname = "tiled_prop_quad_kernel"  # coupling nets on wave pairs beside the encoder pair
        elif flags["NF_cond"] and flags["measurement"] != "CGLOW":
            kname = "tiled_prop2_kernel"       # two roles: flow chain, measurement
        elif flags["measurement"] == "CRNVP" and os.environ.get("NFDPF_CM_TWO_CHAIN", "0") == "1":
            kname = "tiled_prop_cm_kernel"     # two chains: encoder + context folds, coupling nets
        else:
            kname = "tiled_prop_kernel"
    if flags["measurement"] == "CGLOW":
        kname = "cglow_kernel"
    F_EX = F_EXEC.get(cfg_name, F_ALG) if kname.startswith("tiled_prop") else F_ALG
    bound = "mfma" if kname == "cglow_kernel" else "valu"
    if kernel == "tiled" and eng.last_pass:  # the whole pass in one launch: every step's FLOP
        # (no flows on the particle path -- C3's CRNVP, C1's cosine -- is tiled_pass_cm_kernel)
        c3_shape = not flags["NF_dyn"] and not flags["NF_cond"]  # (C1 too: the cosine measurement)
        kname, F_ALG = ("tiled_pass_cm_kernel" if c3_shape else "tiled_pass_kernel"), F_STEP
        F_EX = F_EXEC_STEP.get(cfg_name, F_ALG)
        units, nbytes = B * N * T, B_ALG * B * N * T
    elif kernel == "tiled" and eng.last_fused:  # the whole step in one launch: all of its FLOP
        kname, F_ALG = "tiled_step_fused_kernel", F_STEP
        F_EX = F_EXEC_STEP.get(cfg_name, F_ALG)
    elif front_ms is not None and front_ms > kernel_ms:
        # the step's front launch (gate + resampling + motion [+ nf_dyn inverse]) is the longer
        # one (--force-resample): it is the dominant kernel
        kernel_ms = front_ms
        if kname == "tiled_prop_quad_kernel":  # merged front + nf_dyn inverse (use_merged)
            kname, F_ALG, F_EX = "tiled_fdyn_kernel", F_DYN_INV, F_DYN_INV_EXEC
        else:  # gate + soft resampling + motion: bytes, not FLOP
            kname, F_ALG, F_EX, bound = "tiled_front_kernel", 0.0, 0.0, "hbm"
            nbytes = (B_SOFT + 8.0 + 8.0) * B * N  # resampling + motion's noise / x' writes
    ot_iter_ms, ot_iter_upper = None, False
    if flags["resampler_type"] == "ot" and eng.last_ot_calls:
        ot_iter_ms, ot_iter_upper = ot_iteration_ms(res, T)
        if not ot_iter_upper and ot_iter_ms * eng.last_ot_calls * 10 > kernel_ms * T:  # the Sinkhorn loop dominates
            kname, kernel_ms, bound = "ot_iter_kernel", ot_iter_ms, "valu"
            F_ALG, units = F_OT_PAIR, B * N * N
            F_EX = F_ALG
            # per particle: x~ (8 B) + logw (4) + both potentials read and written (fp64, 32)
            nbytes = 44.0 * B * N
    tag = cfg_name + ("_force" if force else "")
    traffic, traffic_src = pmc_traffic(tag, kname)
    # the pass kernel's template instance that ran: the mode (0 speculative, 1 forced, 2 gated /
    # plan; sharded gated: the cross-rank instance), or the no-flow pass's <MEAS, MFMA, K>
    instance = None
    if kname == "tiled_pass_kernel":
        mode = 1 if force else (2 if (eng.last_gate_pass or eng.last_plan_pass) else 0)
        xr = "true" if (mode == 2 and eng.last_gate_pass and B * (dist.get_world_size() if dist.is_initialized()
                                                                   else 1) != B) else "false"
        instance = f"tiled_pass_kernel<{mode}, {xr}>"
    elif kname == "tiled_pass_cm_kernel":
        meas = {"CRNVP": 1, "cos": 0, "gaussian": 3}.get(flags["measurement"])
        mf = flags["measurement"] == "CRNVP" and os.environ.get("NFDPF_CM_MFMA", "1") != "0"
        k = os.environ.get("NFDPF_CM_K") or ("3" if mf else "2")
        if meas is not None:
            instance = f"tiled_pass_cm_kernel<{meas}, {'true' if mf else 'false'}, {k}>"
    rp_ms, rp_src = rocprof_avg_ms(tag, kname, instance)
    achieved_tf = F_ALG * units / (kernel_ms * 1e-3) / 1e12
    hbm_gbs = nbytes / (kernel_ms * 1e-3) / 1e9
    # bound: the FP32 issue rate of the CU -- VALU for the coupling nets / Sinkhorn
    # (v_pk_fma_f32, v_exp_f32), f32 MFMA + VALU for CGLOW; same 157.3 TFLOP/s peak
    roof = {"bound": bound,
            "achieved": achieved_tf if bound != "hbm" else hbm_gbs,
            "peak": PEAK_FP32_TFLOPS if bound != "hbm" else PEAK_HBM_GBS,
            "unit": "TFLOP/s" if bound != "hbm" else "GB/s",
            "frac": achieved_tf / PEAK_FP32_TFLOPS if bound != "hbm" else hbm_gbs / PEAK_HBM_GBS,
            "traffic": traffic, "traffic_source": traffic_src,
            "kernel": kname, "kernel_avg_ms": kernel_ms,
            # the same kernel's average in the committed rocprofv3 summary of this bench command
            # (profiles/rocprof_<config>.csv; OT: the launches that ran the iteration, not the
            # early-exit tail), beside the live figure
            "kernel_avg_ms_rocprof": rp_ms, "rocprof_source": rp_src,
            "flop_per_unit": F_ALG, "units_per_launch": units,
            "flop_per_unit_executed": F_EX,
            "frac_executed": F_EX * units / (kernel_ms * 1e-3) / 1e12 / PEAK_FP32_TFLOPS,
            "hbm_achieved_GBs": hbm_gbs, "hbm_frac": hbm_gbs / PEAK_HBM_GBS}
    return roof, ot_iter_ms, ot_iter_upper


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--config", default="c2", choices=sorted(CONFIGS))
    ap.add_argument("--force-resample", action="store_true")
    ap.add_argument("--full", action="store_true",
                    help="beside the headline figure: the live roofline of the dominant launch, the resampler on "
                         "its own, the RMSE on informative encodings, the `forced` and `informative` lines and the "
                         "CPU baseline (each in runs of its own after the timed steps; see --no-*)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed pass returned (FilterResult's tensors, "
                         "rank 0's rows) as DIR/<name>.npy; see dump_outputs")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the line's `cpu_baseline`")
    ap.add_argument("--no-forced", action="store_true",
                    help="with --full: skip the line's `forced` object (the same workload with --force-resample, "
                         "timed in a second loop; there for the configurations whose pass takes < 30 ms)")
    ap.add_argument("--no-informative", action="store_true",
                    help="with --full: skip the line's `informative` object (the same workload on informative frame "
                         "encodings, where the ESS gate fires on most steps, timed in its own loop; there for c1-c3)")
    ap.add_argument("--batch", type=int, default=None, help="override B per GPU (exploration only)")
    ap.add_argument("--graph", type=int, default=1,
                    help="1: capture the whole T-step pass (all launches of filtering_pos) in a hipGraph and "
                         "replay it per step (device RNG, soft resampler, one GPU); 0: launch from Python")
    ap.add_argument("--speculate", type=int, default=-1,
                    help="speculative ESS gate (one exchange per pass, engine.FilterConfig.speculate_gate): "
                         "-1 auto (on when sharded or when the pass runs as one launch), 0 off (per-step "
                         "exchange), 1 on")
    ap.add_argument("--kernel", default="tiled", choices=["tiled", "fused"],
                    help="tiled: multi-CU pipeline per step; fused: one workgroup per batch row")
    ap.add_argument("--enc-from-state", action="store_true",
                    help="frame encodings = the particle encoder applied to the true positions (what a "
                         "trained frame encoder approximates): the likelihood peaks near the truth, the "
                         "weights degenerate and the ESS gate fires (cos / CRNVP measurements, 32-wide)")
    args = ap.parse_args()

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    # more ranks than devices (a rehearsal on a one-GPU box) share devices round-robin
    local = local % max(1, torch.cuda.device_count())
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1:
        # "nccl" is RCCL over xGMI; NFDPF_DIST_BACKEND=gloo only for rehearsing several ranks on
        # one device (RCCL refuses two ranks on one GPU)
        backend = os.environ.get("NFDPF_DIST_BACKEND", "nccl")
        dist.init_process_group(backend, device_id=dev if backend == "nccl" else None)

    import dataclasses
    from DPFs import DPF
    from nfdpf.engine import FilterEngine, ShardInfo
    flags, B, N, T, F_STEP, F_PROP = CONFIGS[args.config]
    B = args.batch or B
    torch.manual_seed(2)
    a = make_args(flags, B, N, T, {"force_resample": args.force_resample})
    dpf = DPF(a).to(dev).eval()
    start, state, vel_in, enc = synthetic_disk(B * world, T, 2, a.hiddensize)
    sl = slice(rank * B, (rank + 1) * B)
    start, state, vel_in, enc = (t[sl].to(dev) for t in (start, state, vel_in, enc))
    if args.enc_from_state:
        with torch.no_grad():
            enc = dpf.particle_encoder(state[:, :, :2].float()).contiguous()
    shard = ShardInfo.from_env(B)
    fcfg = dpf.filter_config()
    fcfg.kernel = args.kernel
    if args.speculate >= 0:
        fcfg.speculate_gate = bool(args.speculate)
    run = timed_passes(fcfg, dpf, enc, start, vel_in, shard, args, world, dev)
    res, elapsed, eng, graph, spec = run["res"], run["elapsed"], run["eng"], run["graph"], run["spec"]
    if args.dump_outputs and rank == 0:
        dump_outputs(res, args.dump_outputs)
    if not args.full:  # a plain run stops at the headline figure: none of the lines timed beside it
        args.no_forced = args.no_informative = args.no_cpu_baseline = True
    roof, ot_iter_ms, ot_iter_upper = dominant(args.config, flags, args.kernel, B, N, T, fcfg, run,
                                               args.force_resample) if args.full else (None, None, False)
    front_ms = run["front_ms"]
    # filtering RMSE of the last pass (losses.py:18-31, eval branch) over the whole job
    se = ((res.pred - state[:, :, :2]) ** 2).sum().double()
    cnt = torch.tensor(float(res.pred.numel()), device=dev, dtype=torch.float64)
    if world > 1:
        dist.all_reduce(se)
        dist.all_reduce(cnt)
    rmse = float(torch.sqrt(se / cnt))
    # the same filter on INFORMATIVE frame encodings (the particle encoder at the true
    # positions, what a trained frame encoder approximates): the timed passes' N(0,1) encodings
    # carry no information, so their RMSE is not a filtering-quality number.  One untimed pass
    # on its own engine (the timed engine's speculation state is left alone).
    rmse_inf, enc_inf = None, None
    if args.full and not args.enc_from_state:
        with torch.no_grad():
            enc_inf = dpf.particle_encoder(state[:, :, :2].float()).contiguous()
        res_inf = FilterEngine(fcfg, dpf).run(enc_inf, start, vel_in, shard=shard)
        se = ((res_inf.pred - state[:, :, :2]) ** 2).sum().double()
        if world > 1:
            dist.all_reduce(se)
        rmse_inf = float(torch.sqrt(se / cnt))
    # steps whose ESS gate fired (DPFs.py:165) in the last pass: OT calls are counted on the
    # host by the engine; a soft resample leaves a non-identity index row
    if flags["resampler_type"] == "ot":
        resampled = eng.last_ot_calls
    else:
        ident = (torch.arange(N, device=dev) + N * (shard.row_base + torch.arange(B, device=dev))[:, None])
        resampled = int((res.index != ident[:, None, :]).flatten(2).any(-1).any(0).sum())

    # the resampler on its own (timed with --force-resample as well as gated)
    resample = None
    if not args.full:
        pass
    elif flags["resampler_type"] == "soft":
        rs_ms = soft_resample_ms(res, T)
        rs_gbs = B_SOFT * B * N / (rs_ms * 1e-3) / 1e9
        resample = {"kernel": "soft_resample_kernel (standalone nfdpf_soft_resample on slot T/2)",
                    "avg_ms": rs_ms, "bound": "hbm", "bytes_per_particle": B_SOFT, "achieved_GBs": rs_gbs,
                    "peak_GBs": PEAK_HBM_GBS, "frac": rs_gbs / PEAK_HBM_GBS,
                    "particles_per_s": B * N / (rs_ms * 1e-3)}
    else:
        if ot_iter_ms is None:
            ot_iter_ms, ot_iter_upper = ot_iteration_ms(res, T)
        it_ms = ot_iter_ms
        call10 = ot_call_ms(res, T, 10)
        tf = F_OT_PAIR * B * N * N / (it_ms * 1e-3) / 1e12
        resample = {"kernel": "ot_iter_kernel (one Sinkhorn iteration)", "avg_ms": it_ms, "bound": "valu",
                    "flop_per_pair": F_OT_PAIR, "pairs_per_launch": B * N * N, "achieved_TFLOPs": tf,
                    "peak_TFLOPs": PEAK_FP32_TFLOPS, "frac": tf / PEAK_FP32_TFLOPS,
                    "call_ms_at_10_iterations": call10,
                    "fixed_ms_per_call": None if ot_iter_upper else call10 - 10 * it_ms,
                    "ot_iter_ms_is_upper_bound": ot_iter_upper, "calls_in_last_pass": eng.last_ot_calls}
        if ot_iter_upper:  # the 10 / 20-iteration difference was swamped: no rate from an upper bound
            resample["achieved_TFLOPs"] = resample["frac"] = None
    if front_ms is not None and resample is not None:
        resample["front_launch_ms"] = front_ms  # the step's gate + resampling + motion launch, live

    # the same workload with the resampler every step (--force-resample), timed in its own loop
    # right after: the ESS gate does not fire on the synthetic N(0,1) encodings at init weights,
    # so the headline value times no resampler; this one times one per step
    forced = None
    cheap = args.config in ("c1", "c2", "c3")
    if not args.force_resample and not args.no_forced and cheap:
        fcfg_f = dataclasses.replace(fcfg, force_resample=True)
        run_f = timed_passes(fcfg_f, dpf, enc, start, vel_in, shard, args, world, dev)
        roof_f, _, _ = dominant(args.config, flags, args.kernel, B, N, T, fcfg_f, run_f, True)
        forced = {"value": B * world * N * T * args.steps / run_f["elapsed"], "unit": "particle-steps/s",
                  "ms_per_step": run_f["elapsed"] / args.steps * 1e3, "steps": args.steps,
                  "resampler": flags["resampler_type"], "resampled_steps": T,
                  "execution": "hipGraph replay of the pass" if run_f["graph"] is not None else "Python launches",
                  "roofline": roof_f}

    # the same workload on INFORMATIVE frame encodings (the particle encoder at the true
    # positions: the likelihood peaks near the truth, the weights degenerate and the ESS gate
    # fires on most steps, as with a trained model), timed in its own loop: the gated pass
    # decides and resamples inside the launch there
    informative = None
    if not args.force_resample and not args.enc_from_state and not args.no_informative and cheap and \
            flags["measurement"] in ("cos", "CRNVP"):
        dpf_i, enc_i, enc_note = dpf, enc_inf, "particle encoder at the true positions (--enc-from-state)"
        rmse_note = None
        if flags["measurement"] == "CRNVP":  # C3: the reference init's likelihood is flat -- a trained-like model
            dpf_i, enc_i = trained_like(dpf, state)
            enc_note = ("trained-like CRNVP model (particle encoder ~ N(0, 0.5^2), flows ~ N(0, 0.1^2), seeded: the "
                        "c3_full parity case's) and its encoder at the true positions + 30 % noise")
            rmse_note = ("random weights at trained scales, not a trained model: its sharp likelihood does not peak "
                         "at the truth, so the filter drifts (the line times the OT-firing regime; parity of its "
                         "Sinkhorn calls: scripts/r06_c3_trained_diag.py, test_fullsize_ot_direct)")
        run_i = timed_passes(fcfg, dpf_i, enc_i, start, vel_in, shard, args, world, dev)
        res_i = run_i["res"]
        ident = (torch.arange(N, device=dev) + N * (shard.row_base + torch.arange(B, device=dev))[:, None])
        fired_i = run_i["eng"].last_ot_calls if flags["resampler_type"] == "ot" else \
            int((res_i.index != ident[:, None, :]).flatten(2).any(-1).any(0).sum())
        se_i = ((res_i.pred - state[:, :, :2]) ** 2).sum().double()
        if world > 1:
            dist.all_reduce(se_i)
        eng_i = run_i["eng"]
        informative = {"value": B * world * N * T * args.steps / run_i["elapsed"], "unit": "particle-steps/s",
                       "ms_per_step": run_i["elapsed"] / args.steps * 1e3, "steps": args.steps,
                       "resampled_steps": fired_i, "of_steps": T, "rmse": float(torch.sqrt(se_i / cnt)),
                       **({"rmse_note": rmse_note} if rmse_note else {}),
                       "encodings": enc_note,
                       "execution": ("hipGraph replay of the pass" if run_i["graph"] is not None else "Python launches")
                                    + (", the whole pass as one launch" if eng_i.last_pass else "")
                                    + (", ESS gate decided inside the launch" if eng_i.last_gate_pass else "")
                                    + (", ESS gates following the last exact pass's plan, verified after the pass"
                                       if eng_i.last_plan_pass else ", speculative ESS gate" if run_i["spec"] else ""),
                       "pass_kernel_avg_ms_live": run_i["kernel_ms"] if eng_i.last_pass else None}

    if rank == 0:
        units = B * world * N * T * args.steps
        value = units / elapsed
        out = {
            "metric": "particle-steps/sec (batch x N x T / s) + filtering RMSE, disk-tracking task",
            "value": value, "unit": "particle-steps/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": f"{args.config}: DPF.filtering_pos, " + ", ".join(f"{k}={v}" for k, v in flags.items())
                       + f", N={N}, batch={B} per GPU, seq_len={T}, state_dim=4 (2-D particles), "
                         f"{'forced' if args.force_resample else 'ESS-gated'} resampling, device RNG, "
                         f"{'hipGraph replay of the pass' if graph is not None else 'Python launches'}"
                         + (", the whole pass as one launch" if eng.last_pass else "")
                         + (", ESS gate decided inside the launch" if eng.last_gate_pass else "")
                         + (", ESS gates following the last exact pass's plan, verified once per pass"
                            if eng.last_plan_pass else ", speculative ESS gate verified once per pass" if spec else "")
                         + (", frame encodings = particle encoder(true positions)" if args.enc_from_state else ""),
                       "global_batch": B * world, "num_particles": N, "seq_len": T,
                       "parallelism": f"batch-sharded x{world}"},
            "rmse": rmse,
            "resampled_steps": resampled,
        }
        if args.full:
            out.update({"rmse_informative_encodings": rmse_inf, "roofline": roof, "resample": resample})
        if forced is not None:
            out["forced"] = forced
        if informative is not None:
            out["informative"] = informative
        if not args.no_cpu_baseline and world == 1:
            out["cpu_baseline"] = cpu_baseline(args.config, force=args.force_resample)
        print(json.dumps(out))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
