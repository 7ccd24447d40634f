#!/usr/bin/env python3
"""bench.py — rays/s of the TinyNeRF train step on MI355X (BASELINE.json metric).

    python bench.py --gpus N --steps K --warmup W [--scaling weak|strong] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N --steps K --warmup W

A plain run sets up, runs W warm-up steps, times exactly K steps and prints the contract fields (metric, value, unit,
higher_is_better, dtype, ms_per_step = milliseconds per timed step) with the run's configuration.  --dump-outputs DIR then
also writes what the last timed step returned on rank 0 — loss.npy, comp_rgb.npy (this rank's rays) and params.npy (the flat
fp32 parameters after its Adam update) — all float32; the inputs are seeded, so two runs with the same arguments see the same data.
Everything else below (roofline, per-kernel times, PSNR, the other pipes, precisions, shapes and the CPU baseline) runs only
with --full.

Started from a plain shell with --gpus N > 1, the parent process (before any GPU call) spawns N fresh rank processes
of itself (tnerf/launch.py: RANK/LOCAL_RANK/WORLD_SIZE, MASTER_ADDR=127.0.0.1, a free MASTER_PORT) and relays rank 0's
line; under torch.distributed.run the environment is already set and nothing is spawned.

A "step" is one pass of the training hot path over one batch (reference src/train.py:108-128):
randint pixel indices -> rays of those pixels -> jitter draw -> fused forward (sample, encode, 8x256 MLP,
composite) -> MSE -> backward (dgrad chain, weight-gradient GEMMs, slab reduce) -> [RCCL all-reduce] -> Adam.
Workload (BASELINE.json configs[1]): 100x100 scene, 106 views, L=6 (39 inputs), 8x256 ReLU MLP skip 4,
64 samples/ray, 4096 rays per GPU per step (weak; --scaling strong: 4096 rays in total), fp32.  Data: seeded
synthetic scene (the dataset blob is not available offline), resident in HBM before the timed region.  N>1: one
process per GPU, rays sharded over ranks, one all-reduce(SUM) of the 1.93 MB flat gradient per step.

Rank 0 prints ONE JSON line.  With --full, besides the contract fields it carries
  roofline     — the dominant chain kernel's algorithmic fp32 FLOP/s against the ceiling of the pipe it runs on (x3: the dense
                 fp16 MFMA peak / 3, three partial products per fp32 product), kernel time measured live with HIP events on the
                 launch stream,
  cpu_baseline — the CPU oracle (a port of the reference's fp32 CPU path) timed on this box's host cores on a
                 bounded sample (rank 0, N=1 only): all cores and one thread,
  kernels / psnr — per-kernel times and the PSNR reached (context, not part of the contract),
  rccl_ranks / allreduce — the size of the process group after a real all-reduce and the measured cost of the
                 gradient all-reduce (N>1, or TNERF_FORCE_DIST=1 with one rank),
  fp32_mfma_step — the same step with TNERF_FLAG_FP32_MFMA (plain fp32 fma chains on v_mfma_f32_32x32x2_f32), driver-timed,
  small_batch  — the step at 2048 / 1024 / 512 rays per GPU (the strong-scaling loads of N = 2 / 4 / 8) with per-kernel times, the
                 one-rank RCCL all-reduce of the flat gradient, and the efficiency those two predict,
  bf16         — BASELINE.json configs[3]: the same step with bf16 weights/activations on MFMA,
  ref_default  — the reference's hard-coded model (L=10, 4x128, skip 2, 2048 rays; reference src/train.py:78-79),
  cfg3 / cfg5  — BASELINE.json configs[2] / [4]: 400x400 S=128 (full-image render + train step) and 800x800 S=256
                 random-pose render.
"""
import argparse
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(ROOT, "tiny-nerf-pytorch_amd")
for p in (ROOT, PKG, os.path.join(PKG, "src")):
    if p not in sys.path:
        sys.path.insert(0, p)

L_FREQS, HIDDEN, DEPTH, SKIP = 6, 256, 8, 4
RAYS, SAMPLES, NEAR, FAR, LR = 4096, 64, 2.0, 6.0, 5e-4
PEAK_F32_MFMA_TFLOPS = 157.3        # MI355X_MICROARCH.md: 256 CU x 2.4 GHz x 256 FLOP/clk/CU
PEAK_BF16_MFMA_TFLOPS = 2516.6      # 16x the fp32 MFMA rate (v_mfma_f32_32x32x16_bf16 / _f16: 32 cycles per 32768 FLOP per SIMD)
PEAK_X3_TFLOPS = PEAK_BF16_MFMA_TFLOPS / 3      # an fp32-grade product = 3 fp16 MFMA partial products of two-piece operands
PEAK_HBM_GBS = 8000.0
# what the fp32 fused paths are priced against: the x3 (two-piece fp16) chain unless TNERF_FP32_PIPE selects the plain fp32 MFMA kernels
FP32_PATH_PEAK = PEAK_F32_MFMA_TFLOPS if os.environ.get("TNERF_FP32_PIPE", "").lower() in ("mfma32", "fp32", "mfma") else PEAK_X3_TFLOPS


def mlp_macs(in_dim, hidden, depth, skip):
    """MACs per sample: forward, dgrad (no gradient flows into the encoder), wgrad."""
    fwd = in_dim * hidden + (depth - 1) * hidden * hidden + (in_dim * hidden if skip else 0) + 4 * hidden
    dgrad = (depth - 1) * hidden * hidden + 4 * hidden
    return fwd, dgrad, fwd


def algorithmic_flops(rays=RAYS, samples=SAMPLES, in_dim=6 * L_FREQS + 3, hidden=HIDDEN, depth=DEPTH, skip=SKIP):
    """Per launch of each MFMA kernel."""
    m = rays * samples
    f, d, w = mlp_macs(in_dim, hidden, depth, skip)
    return {"render_fwd": 2 * f * m, "train_fwd": 2 * f * m, "dgrad": 2 * d * m, "wgrad": 2 * w * m}


def kernel_source_sha():
    """Identity of the kernels a PMC capture belongs to: sha256 over csrc/ sources (profiles/*traffic*.json carry it)."""
    h = hashlib.sha256()
    d = os.path.join(PKG, "csrc")
    for n in sorted(os.listdir(d)):
        if n.endswith((".hip", ".hpp", ".h", ".cpp")):
            h.update(n.encode()); h.update(open(os.path.join(d, n), "rb").read())
    return h.hexdigest()[:16]


def measured_traffic(name):
    """HBM bytes per launch from a PMC capture of THIS kernel source (tools/traffic_capture.py writes the file);
    None when no capture of the current sources is committed — never a number from other kernels."""
    try:
        t = json.load(open(os.path.join(ROOT, "profiles", name)))
        if t.get("kernel_source_sha") == kernel_source_sha():
            return t
    except (OSError, ValueError):
        pass
    return None


def host_cores() -> int:
    """CPU threads this process may really use: affinity mask, capped by the cgroup CPU quota."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    return max(1, min(n, int(os.environ.get("TNERF_CPU_THREADS", "32"))))


def cpu_baseline(scene, seconds_budget=20.0):
    """CPU oracle (port of the reference's fp32 CPU path) on the same workload, bounded sample: all host cores on whole
    4096-ray steps, then ONE thread on 512-ray steps (SURVEY §8d CPU protocol)."""
    import numpy as np
    import torch
    from oracle import tnerf_oracle as O
    in_dim = 6 * L_FREQS + 3
    images, poses, focal = torch.from_numpy(scene["images"]), torch.from_numpy(scene["poses"]), float(scene["focal"])
    N, H, W, _ = images.shape
    ro_all, rd_all = O.pinhole_rays(H, W, focal, poses[0])
    pix = images[0].reshape(-1, 3)

    def run(threads, rays, max_iters, budget):
        torch.set_num_threads(threads)
        g = torch.Generator().manual_seed(0)
        params = O.mlp_init(in_dim, HIDDEN, DEPTH, SKIP, g)
        params[2 * DEPTH + 1] += 0.5                       # sigma bias nudge, as on the GPU side
        adam = O.AdamState(params, lr=LR)
        times, t_start = [], time.time()
        for it in range(max_iters):
            inds = torch.randint(0, H * W, (rays,), generator=g)
            u = torch.rand(rays, SAMPLES, generator=g)
            t0 = time.time()
            _, _, grads = O.loss_and_grads(params, SKIP, L_FREQS, ro_all[inds], rd_all[inds], pix[inds], NEAR, FAR, SAMPLES, u)
            adam.step(params, grads)
            if it > 0:
                times.append(time.time() - t0)
            if time.time() - t_start > budget and len(times) >= 2:
                break
        return float(np.median(times)), len(times)

    med, n = run(host_cores(), RAYS, 6, seconds_budget)
    cores = torch.get_num_threads()
    r1 = 512
    med1, n1 = run(1, r1, 4, 10.0)
    torch.set_num_threads(cores)
    return {"value": RAYS / med, "unit": "rays/s", "cores": cores, "kind": "port",
            "sample": f"{n} train steps of {RAYS} rays x {SAMPLES} samples after 1 warm-up (median {med:.2f} s/step), "
                      f"oracle/tnerf_oracle.py in PyTorch CPU fp32, torch {torch.__version__}",
            "one_thread": {"value": r1 / med1, "unit": "rays/s", "cores": 1,
                           "sample": f"{n1} train steps of {r1} rays x {SAMPLES} samples after 1 warm-up (median {med1:.2f} s/step)"}}


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--scaling", choices=("weak", "strong"), default="weak",
                    help="weak: 4096 rays per GPU per step; strong: 4096 rays per step in total (SURVEY §8e)")
    ap.add_argument("--psnr-steps", type=int, default=1000, help="extra untimed steps before reporting PSNR (rank 0 context)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--parity-rng", action="store_true",
                    help="draw pixel indices / jitter with torch.randint / torch.rand on the host side of every step, like the reference "
                         "loop (parity path, one C-ABI call + optimizer call per step) instead of in the kernels from a device-side step "
                         "counter (speed path: the whole step is one hipGraph replay)")
    ap.add_argument("--no-graph", action="store_true", help="speed path without hipGraph capture (4 launches per step)")
    ap.add_argument("--no-bf16", action="store_true", help="skip the bf16-mode section (BASELINE.json configs[3])")
    ap.add_argument("--no-extra", action="store_true", help="skip the ref_default / cfg3 / cfg5 sections")
    ap.add_argument("--ray-tables", action="store_true",
                    help="gather rays/targets from precomputed (N,HW,3) tables like the reference loop (train.py:94-112) "
                         "instead of generating them in the kernel from pose + pixel index")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one returned (loss, comp_rgb, params) as DIR/<name>.npy, float32")
    ap.add_argument("--full", action="store_true",
                    help="also run every context section (roofline, per-kernel times, PSNR, fp32-MFMA pipe, bf16, other shapes, "
                         "scaling, CPU baseline); a plain run times the headline step only")
    return ap.parse_args(argv)


def dump_outputs(out_dir, arrays):
    """--dump-outputs: each tensor of `arrays` as out_dir/<name>.npy in float32."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    for name, t in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), t.detach().float().cpu().numpy())


def main():
    args = parse_args()
    from tnerf import launch
    if args.gpus > 1 and not launch.under_launcher():
        # plain `python bench.py --gpus N`: this parent never touches the GPU; N fresh rank processes do
        sys.exit(launch.spawn_ranks(args.gpus, [os.path.abspath(__file__), *sys.argv[1:]]))
    run(args)


def run(args):
    # The contract is ONE JSON line on stdout.  Libraries chat on fd 1 (RCCL prints a 5-line version banner at
    # communicator creation): point fd 1 at stderr for the duration of the run and restore it for the final print.
    sys.stdout.flush()
    saved_stdout = os.dup(1)
    os.dup2(2, 1)
    import numpy as np
    import torch
    import torch.distributed as dist
    from tnerf import launch

    rank, local, world = launch.read_env(args.gpus)
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a ROCm GPU (the HIP path has no CPU fallback)")
    n_dev = torch.cuda.device_count()
    if local >= n_dev and not os.environ.get("TNERF_SHARE_GPU"):
        raise SystemExit(f"rank {rank}: LOCAL_RANK={local} but only {n_dev} GPU(s) visible")
    local_dev = local % n_dev                                             # TNERF_SHARE_GPU=1: rehearse N ranks on fewer cards (gloo)
    torch.cuda.set_device(local_dev)
    dev = torch.device("cuda", local_dev)
    torch.cuda.set_stream(torch.cuda.Stream(dev))       # a capturable stream of our own for everything below (hipGraph needs a non-NULL stream)
    use_dist = world > 1 or bool(os.environ.get("TNERF_FORCE_DIST"))      # the env var exercises RCCL init with one rank
    backend = os.environ.get("TNERF_DIST_BACKEND", "nccl")                # "nccl" IS RCCL on ROCm
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if "MASTER_PORT" not in os.environ:
            os.environ["MASTER_PORT"] = str(launch.free_port())          # only reachable with one rank
        os.environ.setdefault("RANK", "0"); os.environ.setdefault("WORLD_SIZE", "1")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)

    from tnerf import ops, trainer, lib
    from tnerf import dist as tdist
    from data import make_synthetic_scene
    import nerf as nerf_mod
    import train as train_mod
    from encoding import PositionalEncoding
    from utils import mse2psnr

    scene = make_synthetic_scene(seed=0)
    images = torch.from_numpy(scene["images"]).to(dev)
    poses = torch.from_numpy(scene["poses"]).to(dev)
    focal = float(scene["focal"])
    N, H, W, _ = images.shape

    # rays of this rank: weak = RAYS each; strong = its shard of RAYS (every rank draws the same global batch)
    R_global = world * RAYS if args.scaling == "weak" else RAYS
    lo, hi = tdist.shard_bounds(R_global, rank, world)
    R_local = hi - lo

    encoder = PositionalEncoding(L_FREQS, True).to(dev)

    def make_trainer(precision, L=L_FREQS, hidden=HIDDEN, depth=DEPTH, skip=SKIP, samples=SAMPLES, scene_t=None, rays_global=None, matrix_pipe=None):
        torch.manual_seed(0)                               # identical initial weights on every rank (and in both modes)
        mdl = nerf_mod.TinyNeRF(6 * L + 3, hidden, depth, skip, matrix_pipe=matrix_pipe).to(dev)
        with torch.no_grad():
            # nn.Linear's default init leaves the sigma head at exactly 0 after its ReLU for this 8x256 model
            # (SURVEY.md §7-7): every weight and every gradient would be a zero and the MFMA kernels would be
            # timed on zeros (which clock higher).  Nudge the bias so the network is alive, as the fixtures do.
            mdl.sigma[0].bias += 0.5
        op = trainer.FlatAdam(mdl, lr=LR)
        if args.parity_rng:
            return mdl, op, trainer.FusedTrainer(mdl, op, NEAR, FAR, samples, precision=precision)
        imgs, pss, fc = scene_t if scene_t is not None else (images, poses, focal)
        return mdl, op, trainer.DatasetTrainer(mdl, op, imgs, pss, fc, rays_global if rays_global is not None else R_global, samples, NEAR, FAR,
                                               seed=1234, precision=precision, graph=not args.no_graph)

    model, opt, tr = make_trainer("fp32")

    import rays as rays_mod
    all_o = all_d = None
    if args.ray_tables or (args.full and rank == 0):
        all_o, all_d = [], []
        for i in range(N if args.ray_tables else 1):           # train.py:94-101 (rank 0 needs image 0 for the kernel timings)
            ro, rd = rays_mod.get_rays(H, W, focal, poses[i])
            all_o.append(ro); all_d.append(rd)
        all_o, all_d = torch.stack(all_o), torch.stack(all_d)
    pixels = images.view(N, H * W, 3)
    gen = torch.Generator(device=dev); gen.manual_seed(1234)          # same draws on every rank; rank takes its shard
    state = {"step": 0}
    run_ = {"tr": tr, "R_global": R_global, "lo": lo, "hi": hi, "S": SAMPLES, "pixels": pixels, "poses": poses, "H": H, "W": W,
            "focal": focal, "N": N}

    def one_step():
        c = run_
        tr = c["tr"]
        s = state["step"]; state["step"] += 1
        if not args.parity_rng:
            return tr.step()                               # image index, pixel and jitter draws: in the kernels (device step counter)
        img_i = s % c["N"]
        Rg, lo, hi, S = c["R_global"], c["lo"], c["hi"], c["S"]
        inds = torch.randint(0, c["H"] * c["W"], (Rg,), device=dev, generator=gen)[lo:hi]
        kw = dict(global_rays=Rg, t_rand=torch.rand(Rg, S, device=dev, generator=gen)[lo:hi])
        if args.ray_tables:
            return tr.step(all_o[img_i, inds], all_d[img_i, inds], c["pixels"][img_i, inds], **kw)
        return tr.step_camera(c["poses"][img_i], c["H"], c["W"], c["focal"], inds, c["pixels"][img_i], **kw)

    def fence():
        if use_dist:
            dist.barrier(device_ids=[local_dev]) if backend == "nccl" else dist.barrier()
        torch.cuda.synchronize()

    def timed(n_warm, n_steps):
        """W untimed steps, then EXACTLY K steps between barrier + synchronize fences; MAX over ranks (seconds)."""
        for _ in range(n_warm):
            one_step()
        fence()
        t0 = time.perf_counter()
        for _ in range(n_steps):
            state["last"] = one_step()
        fence()
        dt = time.perf_counter() - t0
        if use_dist:
            t = torch.tensor([dt], dtype=torch.float64, device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt = float(t.item())
        return dt

    def event_ms(fn, reps):
        fn(); torch.cuda.synchronize()
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        for a, b in evs:
            a.record(); fn(); b.record()
        torch.cuda.synchronize()
        return float(np.mean([a.elapsed_time(b) for a, b in evs]))

    dt = timed(args.warmup, args.steps)
    ms_per_step = dt / args.steps * 1e3
    value = R_global * args.steps / dt
    if args.dump_outputs and rank == 0:
        loss_last, comp_last = state["last"]
        dump_outputs(args.dump_outputs, {"loss": loss_last.reshape(-1), "comp_rgb": comp_last, "params": model.hip_state().flat})

    out = {"metric": "rays/s (train step)", "value": value, "unit": "rays/s", "n_gpus": world, "steps": args.steps,
           "warmup": args.warmup, "ms_per_step": ms_per_step, "higher_is_better": True, "scaling": args.scaling,
           "vs_baseline": None,
           "dtype": "f32 values; products = 3 x fp16 MFMA of two-piece operands" if FP32_PATH_PEAK == PEAK_X3_TFLOPS else "f32", "data": "synthetic",
           "dtype_note": ("fp32 values in, out and in every accumulator; the matrix products are APPROXIMATED to fp32 grade on the fp16 "
                          "matrix pipe: every fp32 operand is scaled by a power of two and carried as two fp16 pieces, a*b = a1*b1 (one "
                          "accumulator) + a1*b2 + a2*b1 (a second one), three v_mfma_f32_32x32x16_f16 per 16 k; measured against fp64: "
                          "activations closer than an fp32 fma chain's, every gradient tensor within 2x of the reference's own CPU fp32 error "
                          "(tests/test_gpu_parity.py); the plain fp32-MFMA kernels (TNERF_FP32_PIPE=mfma32 / TinyNeRF(matrix_pipe='fp32_mfma')) "
                          "are timed in fp32_mfma_step")
                         if FP32_PATH_PEAK == PEAK_X3_TFLOPS else "fp32 MFMA (v_mfma_f32_32x32x2_f32)",
           "config": {"workload": "train step: 100x100 synthetic Lego stand-in, 106 views, L=6 posenc, 8x256 ReLU MLP (skip 4), "
                                  f"64 samples/ray, {'4096 rays per GPU' if args.scaling == 'weak' else '4096 rays in total'} per step, "
                                  "Adam, fp32 (BASELINE.json configs[1])",
                      "rays_per_step_global": R_global, "rays_per_gpu": R_local, "samples_per_ray": SAMPLES,
                      "rng": "torch.randint + torch.rand per step (parity path)" if args.parity_rng else
                             "Philox in the kernels from a device-side step counter; step = " + ("eager launches (graph off)" if args.no_graph else
                                                                                                    ("one hipGraph replay" if world == 1 else "two hipGraph replays around one eager all-reduce")),
                      "rays": "precomputed tables + gather" if args.ray_tables else "generated in-kernel from pose + pixel index",
                      "parallelism": f"rays sharded x{world} ({args.scaling}), 1 all-reduce of {opt._st.n_params * 4} B per step" if world > 1 else "single GPU"}}

    # ---- the exchange step on its own: group size after a real all-reduce, and what the all-reduce costs per step
    if use_dist and args.full:
        g = model.hip_state().grad
        probe = torch.ones(1, device=dev)
        dist.all_reduce(probe)
        out["rccl_ranks"] = int(round(float(probe.item())))              # every rank contributed a 1
        out["dist_backend"] = "rccl (torch.distributed nccl)" if backend == "nccl" else backend
        keep = g.clone()
        fence()
        ar_ms = event_ms(lambda: dist.all_reduce(g), 50)
        g.copy_(keep)
        t = torch.tensor([ar_ms], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        out["allreduce"] = {"bytes": int(g.numel() * 4), "us_per_step": float(t.item()) * 1e3, "ranks": dist.get_world_size(),
                            "how": "50 back-to-back all-reduces of the flat gradient between HIP events, max over ranks"}
    elif not use_dist:
        out["rccl_ranks"] = 1

    def kernel_section(st, R, S, precision):
        """Per-kernel times (HIP events on the launch stream = torch's current stream) of the fused step's kernels."""
        import ctypes as C
        inds = torch.randint(0, H * W, (R,), device=dev, generator=gen)
        ro, rd = all_o[0, inds].contiguous(), all_d[0, inds].contiguous()
        u = torch.rand(R, S, device=dev, generator=gen)
        ztab = ops.depth_table(NEAR, FAR, S, dev)
        comp = torch.empty(R, 3, device=dev); gws = torch.full((R, 3), 1e-4, device=dev)
        dep = torch.empty(R, 1, device=dev); acc_ = torch.empty(R, 1, device=dev)
        sp = torch.cuda.current_stream(dev).cuda_stream
        reps = max(5, min(20, args.steps))
        if precision == "fp32":
            plan = st.plan(R * S)
            common = (C.byref(st.desc), st.packed.data_ptr(), ro.data_ptr(), rd.data_ptr(), R, S, ztab.data_ptr(), 1, u.data_ptr(), 0, 0, 1)
            calls = {
                "render_fwd": lambda: lib.call("tnerf_render_fused", *common, comp.data_ptr(), dep.data_ptr(), acc_.data_ptr(), sp),
                "train_fwd": lambda: lib.call("tnerf_train_fwd_fused", *common, comp.data_ptr(), plan.stash.data_ptr(), plan.Mp, sp),
                "dgrad": lambda: lib.call("tnerf_train_dgrad_fused", *common, gws.data_ptr(), plan.stash.data_ptr(), plan.Mp, sp),
                "wgrad": lambda: lib.call("tnerf_wgrad", C.byref(st.desc), plan.stash.data_ptr(), plan.Mp, R * S, plan.jobs.data_ptr(), plan.n_jobs, plan.slabs.data_ptr(), sp),
                "reduce": lambda: lib.call("tnerf_wgrad_reduce", plan.slabs.data_ptr(), plan.reduce.data_ptr(), st.n_params, st.grad.data_ptr(), sp),
            }
            if st.x3_capable and not (st.desc.flags & lib.FLAG_FP32_MFMA):
                # the chain kernels the step actually launches: fp32-grade products on the fp16 matrix pipe (x3)
                for k_ in ("render_fwd", "train_fwd", "dgrad"):
                    calls[k_ + "_fp32_mfma"] = calls[k_]
                x3 = st.repack_x3(("bench", id(st)))
                cx = (C.byref(st.desc), x3.packed.data_ptr()) + common[2:]
                calls["render_fwd"] = lambda: lib.call("tnerf_render_fused_x3", *cx, comp.data_ptr(), dep.data_ptr(), acc_.data_ptr(), sp)
                calls["train_fwd"] = lambda: lib.call("tnerf_train_fwd_fused_x3", *cx, comp.data_ptr(), plan.stash.data_ptr(), plan.Mp, sp)
                calls["dgrad"] = lambda: lib.call("tnerf_train_dgrad_fused_x3", *cx, gws.data_ptr(), plan.stash.data_ptr(), plan.Mp, sp)
            d32 = lib.MlpDesc(st.desc.in_dim, st.desc.hidden, st.desc.depth, st.desc.skip_at, lib.FLAG_FP32_MFMA)
            calls["wgrad_fp32_mfma"] = lambda: lib.call("tnerf_wgrad", C.byref(d32), plan.stash.data_ptr(), plan.Mp, R * S, plan.jobs.data_ptr(), plan.n_jobs, plan.slabs.data_ptr(), sp)
        else:
            b = st.repack_bf16(); bp = b.train_plan(R, S)
            common = (C.byref(st.desc), b.packed.data_ptr(), ro.data_ptr(), rd.data_ptr(), R, S, ztab.data_ptr(), 1, u.data_ptr(), 0, 0, 1)
            calls = {
                "render_fwd": lambda: lib.call("tnerf_render_fused_bf16", *common, comp.data_ptr(), dep.data_ptr(), acc_.data_ptr(), sp),
                "train_fwd": lambda: lib.call("tnerf_train_fwd_fused_bf16", *common, comp.data_ptr(), bp.stash.data_ptr(), sp),
                "dgrad": lambda: lib.call("tnerf_train_dgrad_fused_bf16", *common, gws.data_ptr(), bp.stash.data_ptr(), sp),
                "wgrad": lambda: lib.call("tnerf_wgrad_bf16", C.byref(st.desc), bp.stash.data_ptr(), bp.n_tiles, bp.jobs.data_ptr(), bp.n_jobs, bp.slabs.data_ptr(), sp),
            }
        iso = {name: event_ms(fn, reps) for name, fn in calls.items()}
        # the step's kernels in step order, back to back (what they cost INSIDE a step: the chip's clock depends on what ran just
        # before); events between the launches.  These are the durations the roofline uses; rocprofv3's per-kernel
        # averages of a bench run mix both situations.
        order = [k for k in ("train_fwd", "dgrad", "wgrad", "reduce") if k in calls]
        for k in order:
            calls[k]()
        torch.cuda.synchronize()
        marks = [[torch.cuda.Event(enable_timing=True) for _ in range(len(order) + 1)] for _ in range(reps)]
        for row in marks:
            row[0].record()
            for i, k in enumerate(order):
                calls[k](); row[i + 1].record()
        torch.cuda.synchronize()
        seq = {k: float(np.mean([row[i].elapsed_time(row[i + 1]) for row in marks])) for i, k in enumerate(order)}
        return {name: seq.get(name, ms) for name, ms in iso.items()}, iso

    if rank == 0 and args.full:
        # ---- per-kernel times, live, HIP events on the launch stream (torch's current stream)
        model._ensure_packed()
        kern, kern_iso = kernel_section(model.hip_state(), RAYS, SAMPLES, "fp32")
        fl = algorithmic_flops()
        step_kernels = ("train_fwd", "dgrad", "wgrad")
        x3 = "train_fwd_fp32_mfma" in kern
        chain = ("train_fwd", "dgrad")
        dom = max(chain, key=lambda k: kern[k])                      # the MFMA-bound kernels of the step (wgrad is HBM-bound, below)
        ach = fl[dom] / (kern[dom] * 1e-3) / 1e12
        peak = PEAK_X3_TFLOPS if x3 else PEAK_F32_MFMA_TFLOPS
        cap = measured_traffic("r04_traffic.json")
        out["roofline"] = {"bound": "mfma", "kernel": dom, "achieved": ach, "peak": peak, "unit": "TFLOP/s",
                           "frac": ach / peak,
                           "traffic": cap[dom]["hbm_bytes"] if cap and dom in cap else None,
                           "traffic_source": f"profiles/r04_traffic.json (PMC passes on kernel sources {cap['kernel_source_sha']})" if cap and dom in cap else None,
                           "flops_per_launch": fl[dom], "ms_per_launch": kern[dom],
                           "frac_of_fp32_mfma_peak": ach / PEAK_F32_MFMA_TFLOPS,      # north_star's yardstick (157.3 TFLOP/s): > 1 on the bf16 pipe
                           "note": ("algorithmic fp32 FLOP per launch; each product runs as 3 fp16 MFMA partial products (two-piece operands), "
                                    "so the ceiling is the dense fp16 MFMA peak / 3 = %.1f TFLOP/s; executed fp16 rate = 3 x achieved" % PEAK_X3_TFLOPS)
                                   if x3 else "fp32 MFMA"}
        for k_ in list(kern):
            if k_.endswith("_fp32_mfma"):
                fl[k_] = fl[k_[:-len("_fp32_mfma")]]
        def _peak(k_):
            return PEAK_F32_MFMA_TFLOPS if (k_.endswith("_fp32_mfma") or not x3) else PEAK_X3_TFLOPS
        out["kernels"] = {k: {"ms": kern[k], "tflops": (fl[k] / (kern[k] * 1e-3) / 1e12) if k in fl else None,
                              "mfma_frac": (fl[k] / (kern[k] * 1e-3) / 1e12 / _peak(k)) if k in fl else None,
                              "mfma_peak": _peak(k) if k in fl else None, "ms_alone": kern_iso[k]} for k in kern}
        for k_ in out["kernels"]:
            if cap and k_ in cap and isinstance(cap[k_], dict):
                out["kernels"][k_]["traffic"] = cap[k_]["hbm_bytes"]
        out["kernels"]["_timing"] = ("ms: HIP events between the launches of train_fwd -> dgrad -> wgrad -> reduce issued back to back in step "
                                     "order (the other entries: alone); ms_alone: the same launch repeated on its own")
        # the weight-gradient kernel runs its products on the fp16 matrix pipe too (3 partial products): priced against both of its bounds
        m_ = RAYS * SAMPLES
        wg_bytes = m_ * 4 * ((HIDDEN + 64) * 2 + (DEPTH - 1) * 2 * HIDDEN + 32 + HIDDEN)        # every job class reads its A and B rows of the stash once
        for k_ in ("wgrad", "wgrad_fp32_mfma"):
            out["kernels"][k_].update(algorithmic_hbm_bytes=wg_bytes, hbm_gbs=wg_bytes / (kern[k_] * 1e-3) / 1e9,
                                      hbm_frac=wg_bytes / (kern[k_] * 1e-3) / 1e9 / PEAK_HBM_GBS,
                                      traffic=cap[k_]["hbm_bytes"] if cap and k_ in cap else None)
        out["kernels"]["wgrad"]["matrix_pipe"] = "fp16 MFMA, fp32 operands as two scaled fp16 pieces (3 of 4 partial products), fp32 accumulate"
        out["kernels"]["wgrad_fp32_mfma"]["matrix_pipe"] = "fp32 MFMA (TNERF_FLAG_FP32_MFMA)"
        if args.scaling == "weak" or world == 1:
            step_flops = sum(fl[k] for k in step_kernels)
            out["step_mfma_frac"] = step_flops / (ms_per_step * 1e-3) / 1e12 / peak
            out["step_minus_big3_us"] = (ms_per_step - sum(kern[k] for k in step_kernels)) * 1e3

    if args.full:
        held = make_synthetic_scene(n_images=8, seed=1)           # eight cameras on the same scene that are not in the training set
        h_images = torch.from_numpy(held["images"]).to(dev); h_poses = torch.from_numpy(held["poses"]).to(dev)

    def psnr_block(mdl, extra=None):
        """Keep training (untimed), then minibatch PSNR, the full-image PSNR of one training view, and — the statistic the bf16
        tolerance of BASELINE configs[3] is checked on, as tests/test_gpu_parity.py::test_bf16_trainer_tracks_fp32_training does —
        the HELD-OUT PSNR: mean over 8 unseen views, averaged over the last 5 checkpoints (one checkpoint's value moves by ~0.1 dB
        from step to step)."""
        losses, ckpts = [], []
        every = max(1, args.psnr_steps // 20)
        for i in range(args.psnr_steps):
            loss, _ = one_step()
            if i >= args.psnr_steps - 20:
                losses.append(loss.clone())
            left = args.psnr_steps - 1 - i
            if rank == 0 and left % every == 0 and left // every < 5:
                ps = [float(mse2psnr(torch.mean((train_mod.render_one(mdl, encoder, H, W, focal, h_poses[k], dev, n_samples=SAMPLES, near=NEAR, far=FAR) - h_images[k]) ** 2)))
                      for k in range(h_poses.shape[0])]
                ckpts.append(sum(ps) / len(ps))
        mb = torch.stack(losses).mean()
        if use_dist:
            dist.all_reduce(mb)                                     # each rank's loss is its shard's share of the global mean
        if rank != 0:
            return None
        img = train_mod.render_one(mdl, encoder, H, W, focal, poses[N - 1], dev, n_samples=SAMPLES, near=NEAR, far=FAR)
        full = float(mse2psnr(torch.mean((img - images[N - 1]) ** 2)))
        return {"train_minibatch_db": float(mse2psnr(mb)), "full_image_view105_db": full, "after_steps": state["step"],
                "heldout_8_views_last_5_checkpoints_db": sum(ckpts) / len(ckpts), "heldout_checkpoints_db": [round(c, 3) for c in ckpts],
                "heldout_checkpoint_every_steps": every}, img

    # ---- PSNR context
    if args.full and args.psnr_steps > 0:
        r = psnr_block(model)
        if r:
            out["psnr"] = r[0]; img_f32 = r[1]
        # context for `value`: the SAME protocol (W warm-up + K timed steps) on the network as it is now, after the PSNR block's training.
        # `value` above times the first steps of a freshly initialised network; as the network learns, most activations and nearly all
        # activation gradients become exact zeros, the matrix pipe draws less power and the chip clocks higher ("Where it stands")
        dt_tr = timed(args.warmup, args.steps)
        out["trained_network_step"] = {"ms_per_step": dt_tr / args.steps * 1e3, "value": R_global * args.steps / dt_tr, "unit": "rays/s",
                                       "after_steps": state["step"] - args.warmup - args.steps,
                                       "note": "same trainer, same W + K protocol as `value`, on the trained weights: the step's time depends on the data"}

    # ---- the same step on the plain fp32-MFMA kernels (TNERF_FLAG_FP32_MFMA): what the x3 pipe buys, driver-timed like `value`
    if args.full and not args.no_extra and FP32_PATH_PEAK == PEAK_X3_TFLOPS:
        m32, o32, t32 = make_trainer("fp32", matrix_pipe="fp32_mfma")
        run_["tr"] = t32
        gen.manual_seed(1234); state["step"] = 0
        d32 = timed(args.warmup, args.steps)
        f_, dg_, wg_ = mlp_macs(6 * L_FREQS + 3, HIDDEN, DEPTH, SKIP)
        out["fp32_mfma_step"] = {"matrix_pipe": "v_mfma_f32_32x32x2_f32: fp32 fma chains in the chain kernels and the weight-gradient kernel",
                                 "ms_per_step": d32 / args.steps * 1e3, "value": R_global * args.steps / d32, "unit": "rays/s",
                                 "mfma_frac": 2 * (f_ + dg_ + wg_) * R_local * SAMPLES / (d32 / args.steps) / 1e12 / PEAK_F32_MFMA_TFLOPS,
                                 "mfma_peak": PEAK_F32_MFMA_TFLOPS, "x3_speedup": d32 / dt}
        # the like-for-like figure on the pipe north_star names (fp32 MFMA), beside `value`
        out["fp32_mfma_value"] = out["fp32_mfma_step"]["value"]
        out["fp32_mfma_ms_per_step"] = out["fp32_mfma_step"]["ms_per_step"]
        out["frac_of_fp32_mfma_peak"] = out["fp32_mfma_step"]["mfma_frac"]
        run_["tr"] = tr
        del m32, o32, t32

    # ---- N > 1: the OTHER scaling mode and what the exchange costs, in the same line (a SCALE run needs no extra flags).
    # `value` above is the contract number (weak unless --scaling strong).  Here: the same step with the global batch fixed at 4096 rays
    # (strong) resp. 4096 per rank (weak), and both again WITHOUT the all-reduce — the difference is the exposed (non-overlapped) part of
    # the exchange; allreduce.us_per_step above is the collective on its own.
    if args.full and world > 1 and not args.no_extra and not args.parity_rng:
        def other_mode():
            res = {}
            for mode in ("weak", "strong"):
                Rg = world * RAYS if mode == "weak" else RAYS
                lo_, hi_ = tdist.shard_bounds(Rg, rank, world)
                if hi_ - lo_ < 1:
                    res[mode] = {"error": f"{Rg} rays do not split over {world} ranks"}
                    continue
                mdl, op, t_ = make_trainer("fp32", rays_global=Rg)
                run_.update(tr=t_, R_global=Rg, lo=lo_, hi=hi_)
                state["step"] = 0
                d_ex = timed(args.warmup, args.steps)
                t_.skip_exchange_for_timing = True
                d_no = timed(args.warmup, args.steps)
                t_.skip_exchange_for_timing = False
                res[mode] = {"value": Rg * args.steps / d_ex, "unit": "rays/s", "ms_per_step": d_ex / args.steps * 1e3, "rays_per_step_global": Rg,
                             "rays_per_gpu": hi_ - lo_, "ms_per_step_without_allreduce": d_no / args.steps * 1e3,
                             "exposed_allreduce_us": (d_ex - d_no) / args.steps * 1e6}
                del mdl, op, t_
            run_.update(tr=tr, R_global=R_global, lo=lo, hi=hi)
            res["how"] = ("each mode: W warm-up + K timed steps between barrier + synchronize fences, max over ranks, with the all-reduce and (ranks' weights "
                          "then diverge: timing only, on throw-away models) without it; one un-bucketed all-reduce of the flat gradient per step between two "
                          "captured graphs — bucketing it behind the weight-gradient kernel does not pay in this design (DESIGN.md, multi-GPU)")
            return res
        try:
            out["scaling_modes"] = other_mode()
        except Exception as e:
            out["scaling_modes"] = {"error": f"{type(e).__name__}: {e}"}

    # ---- strong-scaling loads on one GPU: the step at 2048 / 1024 / 512 rays (what each of N = 2 / 4 / 8 ranks runs when 4096 rays are
    # sharded) + the cost of an RCCL all-reduce of the flat gradient in a one-rank group -> the efficiency these predict
    if args.full and not args.no_extra and world == 1 and rank == 0:
        def small_batch():
            own_group = False
            if not dist.is_initialized():
                os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
                os.environ["MASTER_PORT"] = str(launch.free_port())
                os.environ.setdefault("RANK", "0"); os.environ.setdefault("WORLD_SIZE", "1")
                dist.init_process_group("nccl", device_id=dev)
                own_group = True
            g = model.hip_state().grad
            keep = g.clone()
            ar_us = event_ms(lambda: dist.all_reduce(g), 50) * 1e3
            g.copy_(keep)
            nbytes = int(g.numel() * 4)
            res = {"allreduce_one_rank": {"bytes": nbytes, "us": ar_us,
                                          "how": "50 back-to-back RCCL all-reduces of the flat gradient in a one-rank group between HIP events: "
                                                 "the launch + kernel floor, no link traffic"},
                   "rays_per_gpu": {}}
            base_ms = ms_per_step
            for n_ranks, rays in ((2, 2048), (4, 1024), (8, 512)):
                mdl, op, t_ = make_trainer("fp32", rays_global=rays)
                run_.update(tr=t_, R_global=rays, lo=0, hi=rays)
                d_ = timed(10, max(50, args.steps))
                ms = d_ / max(50, args.steps) * 1e3
                mdl._ensure_packed()
                kern_, _ = kernel_section(mdl.hip_state(), rays, SAMPLES, "fp32")
                # ring all-reduce of `nbytes` over n_ranks on xGMI: 2 (n-1)/n of the bytes cross each link; one link ~ 153 GB/s peak, 70 % assumed
                link_us = 2.0 * (n_ranks - 1) / n_ranks * nbytes / (153e9 * 0.7) * 1e6
                ar_pred = ar_us + link_us
                res["rays_per_gpu"][str(rays)] = {
                    "ms_per_step": ms, "kernels_ms": {k: kern_[k] for k in ("train_fwd", "dgrad", "wgrad", "reduce") if k in kern_},
                    "for_n_gpus": n_ranks, "allreduce_us_model": ar_pred,
                    "predicted_strong_efficiency": base_ms / (n_ranks * (ms + ar_pred * 1e-3)),
                    "predicted_strong_efficiency_allreduce_hidden": base_ms / (n_ranks * ms)}
                del mdl, op, t_
            res["weak_predicted_efficiency"] = {str(n): base_ms / (base_ms + (ar_us + 2.0 * (n - 1) / n * nbytes / (153e9 * 0.7) * 1e6) * 1e-3) for n in (2, 4, 8)}
            res["model"] = ("t_N = t_step(4096/N rays, measured here) + all-reduce(N) with all-reduce(N) = one-rank RCCL floor (measured here) + "
                            "2 (N-1)/N x bytes / (0.7 x 153 GB/s) ring term; efficiency = t_1(4096 rays) / (N t_N).  The step at N > 1 runs as two "
                            "captured graphs around one eager all-reduce (tnerf/trainer.py)")
            run_.update(tr=tr, R_global=R_global, lo=lo, hi=hi)
            if own_group:
                dist.destroy_process_group()
            return res
        try:
            out["small_batch"] = small_batch()
        except Exception as e:
            out["small_batch"] = {"error": f"{type(e).__name__}: {e}"}
            run_.update(tr=tr, R_global=R_global, lo=lo, hi=hi)

    # ---- bf16 mode (BASELINE.json configs[3]): same initial weights, same pixel / jitter stream, same step counts
    if args.full and not args.no_bf16:
        model16, opt16, tr16 = make_trainer("bf16")
        run_["tr"] = tr16
        gen.manual_seed(1234); state["step"] = 0
        dt16 = timed(args.warmup, args.steps)
        b16 = {"dtype": "bf16 operands, fp32 accumulate / compositing / master weights", "ms_per_step": dt16 / args.steps * 1e3,
               "value": R_global * args.steps / dt16, "unit": "rays/s", "speedup_vs_fp32_step": dt / dt16}
        if rank == 0:
            st = model16.hip_state()
            k16, k16_alone = kernel_section(st, RAYS, SAMPLES, "bf16")
            fl = algorithmic_flops()
            # algorithmic HBM bytes of the stash streams: 2 KB per (32-sample tile, 32-feature tile) of bf16
            # activations / activation gradients; the forward also writes the ReLU bits and the head outputs
            NT = HIDDEN // 32
            tiles = RAYS * ((SAMPLES + 31) // 32)
            wg_tiles = (NT + 2) + (DEPTH - 1) * 2 * NT + ((NT + 2) if SKIP else 0) + (1 + NT)     # sum over job classes of A + B feature tiles
            hbm = {"train_fwd": tiles * ((2 + DEPTH * NT) * 2048 + DEPTH * (HIDDEN // 64) * 256 + 512),
                   "dgrad": tiles * (DEPTH * NT + 1) * 2048,
                   "wgrad": tiles * wg_tiles * 2048}
            cap16 = measured_traffic("r04_traffic_bf16.json") or {}
            kern16 = {}
            for name, ms in k16.items():
                kern16[name] = {"ms": ms, "ms_alone": k16_alone[name], "tflops": fl[name] / (ms * 1e-3) / 1e12,
                                "mfma_frac": fl[name] / (ms * 1e-3) / 1e12 / PEAK_BF16_MFMA_TFLOPS}
                if name in hbm:
                    kern16[name].update(algorithmic_hbm_bytes=hbm[name], hbm_gbs=hbm[name] / (ms * 1e-3) / 1e9,
                                        hbm_frac=hbm[name] / (ms * 1e-3) / 1e9 / PEAK_HBM_GBS,
                                        traffic=cap16.get(name, {}).get("hbm_bytes") if isinstance(cap16.get(name), dict) else None)
            b16["kernels"] = kern16
            b16["roofline"] = {"bound": "hbm", "kernel": "wgrad", "achieved": kern16["wgrad"]["hbm_gbs"], "peak": PEAK_HBM_GBS,
                               "unit": "GB/s", "frac": kern16["wgrad"]["hbm_frac"], "traffic": kern16["wgrad"]["traffic"]}
            if args.scaling == "weak" or world == 1:
                b16["step_minus_big3_us"] = (b16["ms_per_step"] - sum(k16[k] for k in ("train_fwd", "dgrad", "wgrad"))) * 1e3
        if args.psnr_steps > 0:
            r = psnr_block(model16)
            if r:
                p16, img = r
                st16 = model16._ensure_packed()
                img16 = ops.render_camera_fused_bf16(st16, poses[N - 1], H, W, focal, 0, H * W, NEAR, FAR, SAMPLES)[0].reshape(H, W, 3).clamp(0, 1)
                p16.update(full_image_rendered_in_bf16_db=float(mse2psnr(torch.mean((img16 - images[N - 1]) ** 2))),
                           max_abs_rgb_bf16_vs_fp32_render=float((img16 - img).abs().max()))
                if "psnr" in out:
                    # the comparison BASELINE configs[3] asks for (|dPSNR| <= 0.1 dB, held-out): means over 8 unseen views x 5 checkpoints
                    p16["delta_heldout_db_vs_fp32"] = p16["heldout_8_views_last_5_checkpoints_db"] - out["psnr"]["heldout_8_views_last_5_checkpoints_db"]
                    p16["delta_tolerance_db"] = 0.1
                    # (one checkpoint of ONE training view, for continuity with earlier rounds' lines: chaotic to +-0.2 dB)
                    p16["delta_full_image_view105_db_vs_fp32"] = p16["full_image_view105_db"] - out["psnr"]["full_image_view105_db"]
                b16["psnr"] = p16
        out["bf16"] = b16
        run_["tr"] = tr
        del model16, opt16, tr16

    # ---- the other shapes of BASELINE.json / the reference, driver-visible (context; every rank takes part when N > 1)
    if args.full and not args.no_extra:
        def section(fn):
            try:
                return fn()
            except Exception as e:                                   # a context section must not take the contract line down
                return {"error": f"{type(e).__name__}: {e}"}

        def train_shape(L, hidden, depth, skip, rays, samples, scene_t, steps, warm):
            """ms/step of the fused train step for another (model, batch) shape, fp32 and bf16, this rank's share."""
            res = {}
            imgs, pss, fc = scene_t
            n, h, w, _ = imgs.shape
            Rg = world * rays if args.scaling == "weak" else rays
            l0, h0 = tdist.shard_bounds(Rg, rank, world)
            for prec in ("fp32", "bf16"):
                mdl, op, t_ = make_trainer(prec, L, hidden, depth, skip, samples, scene_t=scene_t, rays_global=Rg)
                run_.update(tr=t_, R_global=Rg, lo=l0, hi=h0, S=samples, pixels=imgs.view(n, h * w, 3), poses=pss, H=h, W=w, focal=fc, N=n)
                d_ = timed(warm, steps)
                f, dg, wg = mlp_macs(6 * L + 3, hidden, depth, skip)
                flops = 2 * (f + dg + wg) * (h0 - l0) * samples
                peak = FP32_PATH_PEAK if prec == "fp32" else PEAK_BF16_MFMA_TFLOPS
                res[prec] = {"ms_per_step": d_ / steps * 1e3, "rays_per_s": Rg * steps / d_,
                             "mfma_frac": flops / (d_ / steps) / 1e12 / peak}
                del mdl, op, t_
            run_.update(tr=tr, R_global=R_global, lo=lo, hi=hi, S=SAMPLES, pixels=pixels, poses=poses, H=H, W=W, focal=focal, N=N)
            return res

        def render_shape(mdl, enc, h, w, fc, pose_list, samples, prec):
            """Full-image render (render_one_sharded: pixels sharded over ranks, all-gathered), rays/s over all poses."""
            train_mod.render_one_sharded(mdl, enc, h, w, fc, pose_list[0], dev, n_samples=samples, near=NEAR, far=FAR, precision=prec)
            fence()
            t0 = time.perf_counter()
            for p_ in pose_list:
                img_ = train_mod.render_one_sharded(mdl, enc, h, w, fc, p_, dev, n_samples=samples, near=NEAR, far=FAR, precision=prec)
            fence()
            d_ = time.perf_counter() - t0
            if use_dist:
                t = torch.tensor([d_], dtype=torch.float64, device=dev)
                dist.all_reduce(t, op=dist.ReduceOp.MAX)
                d_ = float(t.item())
            rays_s = h * w * len(pose_list) / d_
            f, _, _ = mlp_macs(enc.out_dim, mdl.hidden, mdl.depth, mdl.skip_at)
            peak = FP32_PATH_PEAK if prec == "fp32" else PEAK_BF16_MFMA_TFLOPS
            return {"ms_per_image": d_ / len(pose_list) * 1e3, "rays_per_s": rays_s, "images": len(pose_list),
                    "mfma_frac": 2 * f * samples * rays_s / world / 1e12 / peak,
                    "hbm_frac": 12.0 * rays_s / world / 1e9 / PEAK_HBM_GBS, "finite": bool(torch.isfinite(img_).all())}

        scene_t = (images, poses, focal)
        # the reference's own hard-coded model and batch (reference src/train.py:23,78-79): L=10, 4x128, skip 2, 2048 rays
        out["ref_default"] = section(lambda: dict(
            workload="train step: reference default model L=10 (63 inputs), 4x128 skip 2, 2048 rays x 64 samples, 100x100 scene",
            **train_shape(10, 128, 4, 2, 2048, 64, scene_t, max(20, args.steps), 10)))

        def cfg3():
            sc = make_synthetic_scene(n_images=8, H=400, W=400, focal=4 * 138.88887889922103, seed=0)
            st_ = (torch.from_numpy(sc["images"]).to(dev), torch.from_numpy(sc["poses"]).to(dev), float(sc["focal"]))
            r = {"workload": "400x400 analytic re-render of the synthetic scene (8 views), 128 samples/ray, 8x256 L=6: train step of 4096 "
                             "rays per GPU and full-image render of 160,000 rays sharded over the ranks (BASELINE.json configs[2])"}
            r["train"] = train_shape(L_FREQS, HIDDEN, DEPTH, SKIP, RAYS, 128, st_, 10, 3)
            r["render"] = {p_: render_shape(model, encoder, 400, 400, st_[2], [st_[1][i] for i in range(2)], 128, p_) for p_ in ("fp32", "bf16")}
            return r
        out["cfg3"] = section(cfg3)

        def cfg5():
            g5 = torch.Generator().manual_seed(5)
            ps = []
            for _ in range(8):                                       # SURVEY §8d cfg 5: seeded QR of N(0,1) 3x3, det +1, origin on the radius-4 sphere
                q, r_ = torch.linalg.qr(torch.randn(3, 3, generator=g5))
                q = q * torch.sign(torch.diagonal(r_))
                if torch.det(q) < 0:
                    q[:, 2] = -q[:, 2]
                o = torch.nn.functional.normalize(torch.randn(3, generator=g5), dim=0) * 4.0
                m = torch.eye(4); m[:3, :3] = q; m[:3, 3] = o
                ps.append(m.to(dev))
            torch.manual_seed(0)
            m5 = nerf_mod.TinyNeRF(encoder.out_dim, HIDDEN, DEPTH, SKIP).to(dev)
            with torch.no_grad():
                m5.sigma[0].bias += 0.5
            return {"workload": "800x800, 256 samples/ray, random poses, seed-0 weights with sigma bias +0.5, render only, 640,000 rays "
                                "per image sharded over the ranks (BASELINE.json configs[4]); the fused kernel moves 12 B/ray of HBM, so "
                                "the bound is MFMA, not HBM",
                    "render": {"fp32": render_shape(m5, encoder, 800, 800, 4 * 138.88887889922103 * 2, ps[:2], 256, "fp32"),
                               "bf16": render_shape(m5, encoder, 800, 800, 4 * 138.88887889922103 * 2, ps, 256, "bf16")}}
        out["cfg5"] = section(cfg5)

    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(scene)
    fence()
    if use_dist:
        dist.destroy_process_group()
    sys.stdout.flush()
    os.dup2(saved_stdout, 1)
    os.close(saved_stdout)
    if rank == 0:
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
