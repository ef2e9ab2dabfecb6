#!/usr/bin/env python3
"""Benchmark of the SMART-Vocoder inference path on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--batch 16] [--frames 512] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

One "step" = SynthesizerTrn.infer over one batch of synthetic mels (BASELINE.json configs[1]:
iitp_base, batch 16 x 512 frames per GPU, 22.05 kHz), inputs resident in HBM.  Metric: audio samples/s
(whole job).  Weak scaling: every rank runs its own 16x512 shard; rank 0 owns the job's batch
(scattered over RCCL before the timed region) and receives all waveforms (gather inside the timed region).
Prints ONE JSON line on rank 0.

A plain run sets up, warms up, times the K steps, writes --dump-outputs and prints the line; the roofline block it carries is
priced from the library's counters of the timed region.  --full adds, after the timed region, everything that takes runs of
its own: at N=1 the dominant kernel's per-launch time, the live HBM-traffic and MFMA-count passes (rocprofv3 --pmc child
runs), the other single-GPU configurations, the CPU baseline and the whole-batch parity check against the CPU oracle (exit 4
when it fails); at N>1 the separately timed input scatter and parallel.infer_sharded.  --no-cpu-baseline, --no-pmc and
--no-other-configs drop single parts of --full.

--dump-outputs DIR: after the timed steps rank 0 writes what the last timed step returned as DIR/<name>.npy (float32):
at N=1 every output of `infer` (o, x_mask, z, z_p, m_p, logs_p), at N>1 the gathered waveform o.  Inputs and weights are
seeded, so two builds run with the same arguments can be compared array for array.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FLOP_PER_SAMPLE = 2568280.0          # 2*MAC of the 184 convolutions per output sample
FP32_MFMA_PEAK_TFLOPS = 157.3        # /opt/skills/guides/MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32 peak
SAMPLE_RATE = 22050
ROUND_TAG = "r05"                     # only PMC traffic files of this round's code are quoted


def _cpu_info():
    model, phys = "unknown", None
    try:
        cores = set()
        phys_id = core_id = None
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name") and model == "unknown":
                model = line.split(":", 1)[1].strip()
            elif line.startswith("physical id"):
                phys_id = line.split(":", 1)[1].strip()
            elif line.startswith("core id"):
                core_id = line.split(":", 1)[1].strip()
            elif not line.strip():
                if phys_id is not None and core_id is not None:
                    cores.add((phys_id, core_id))
                phys_id = core_id = None
        phys = len(cores) or None
    except Exception:   # noqa: BLE001
        pass
    return model, phys


def cpu_baseline(sd_np, seed, keep=None):
    """the CPU oracle (oracle/vocoder_oracle.py, a restatement of the reference forward: kind "port")
    timed on the host cores with 1 warm-up + best of 3, on C2 (16 x 512, the bench workload: `value`) and on C1 (1 x 200,
    the reference notebook's shape).  torch's intra-op thread count is chosen by a short probe (more threads than ~16-32
    make oneDNN's small convolutions slower on a 2x64-core host, profiles/r01_cpu_threads_probe.txt); `cores` is
    the count actually used; the CPU model and physical core count are recorded."""
    from oracle import vocoder_oracle as O
    from cases import sw
    avail = os.cpu_count() or 1
    try:
        avail = len(os.sched_getaffinity(0))
    except Exception:   # noqa: BLE001
        pass
    model, phys = _cpu_info()
    sd = {k: torch.from_numpy(v) for k, v in sd_np.items()}
    t_all = time.perf_counter()

    def run(mel, ln, eps, tag=None):
        t0 = time.perf_counter()
        o, *_ = O.infer(sd, mel, ln, eps, 0.667)
        dt = time.perf_counter() - t0
        if keep is not None and tag is not None:
            keep[tag] = o                      # the oracle's waveform of the bench workload: bench.py's parity block checks the GPU against it
        return dt, o.numel()

    with torch.no_grad():
        pm = torch.from_numpy(sw.synthetic_mel(seed, 1, 96)); pe = torch.from_numpy(sw.synthetic_eps(seed, 1, 96))
        best, cores = None, 1
        for n in sorted({min(avail, c) for c in (8, 16, 32, 64)}):
            torch.set_num_threads(n)
            run(pm[:, :, :16], torch.tensor([16]), pe[:, :, :16])      # thread-pool warm-up
            dt, _ = run(pm, torch.tensor([96]), pe)
            if best is None or dt < best:
                best, cores = dt, n
        torch.set_num_threads(cores)
        rec = {}
        for tag, (B, T) in (("c2", (16, 512)), ("c1", (1, 200))):
            mel = torch.from_numpy(sw.synthetic_mel(seed, B, T)); eps = torch.from_numpy(sw.synthetic_eps(seed, B, T))
            ln = torch.full((B,), T, dtype=torch.int64)
            wb = max(1, B // 4)
            run(mel[:wb], ln[:wb], eps[:wb])                                  # warm-up (same T, a quarter of the batch)
            times = []
            for rep in range(3):
                dt, n = run(mel, ln, eps, tag if rep == 0 else None)
                times.append(dt)
            rec[tag] = dict(value=n / min(times), unit="samples/s", shape=f"{B}x{T}", best_s=min(times), all_s=[round(t, 3) for t in times])
            if tag == "c2" and phys and min(avail, phys) != cores:
                # SURVEY.md 8(d) names "all physical host cores": the same workload once at that thread count, beside the best one
                nall = min(avail, phys)
                torch.set_num_threads(nall)
                run(mel[:wb], ln[:wb], eps[:wb])
                dt, n = run(mel, ln, eps)
                rec["c2_all_cores"] = dict(value=n / dt, unit="samples/s", threads=nall, shape=f"{B}x{T}", s=round(dt, 3), runs=1)
                torch.set_num_threads(cores)
    return dict(value=rec["c2"]["value"], unit="samples/s", cores=cores, kind="port",
                sample=f"16x512 frames (the bench workload, whole batch), 1 warm-up + best of 3 = {rec['c2']['best_s']:.2f} s; "
                       f"{cores} of {avail} host threads (best of an 8/16/32/64 probe), torch {torch.__version__} fp32 oneDNN",
                cpu_model=model, physical_cores=phys, logical_cpus=avail, c1_1x200=rec["c1"], c2_16x512=rec["c2"],
                c2_16x512_all_physical_cores=rec.get("c2_all_cores"),
                cores_note=f"SURVEY.md 8(d) asks for all physical cores ({phys}); {cores} threads measured FASTER than more in the probe "
                           "(oneDNN's small convolutions stop scaling), so the best thread count is the one reported",
                protocol="SURVEY.md 8(d): 1 warm-up + best of 3, C1 and C2", wall_s=round(time.perf_counter() - t_all, 1))


def dominant_kernel_probe(net, mel, ln, eps, steps=2):
    """Per-launch duration of the dominant kernel, measured live with HIP events on the launch stream by the library's
    event profiler (every GEMM-family launch bracketed by hipEventRecord): the grouped launch of the C=128 stage's
    three undilated convolutions k=11/7/3 (conv_wino4_group_kernel<1,4,0,true>: k=11/7 in Winograd F(4,4) form, k=3 in F(4,3);
    conv_wino_group_kernel<1,4>, F(2,3), when SVOC_WINO_F4=0; conv_group_kernel when
    SVOC_WINO=0).  Runs after the timed region."""
    from smart_vocoder_amd import _native
    _native.profile_enable(True)
    with torch.no_grad():
        for _ in range(steps):
            net.infer(mel, ln, noise_scale=0.667, eps=eps)
    torch.cuda.synchronize()
    rep = _native.profile_report()
    _native.profile_enable(False)
    best = None
    for line in rep.splitlines():
        if not (line.startswith("group ") or line.startswith("winoG ") or line.startswith("wino4G ")):
            continue
        f = line.split()
        n, total_ms, mean_us, tfl = int(f[-4]), float(f[-3]), float(f[-2]), float(f[-1])
        if best is None or total_ms > best["total_ms"]:
            best = dict(desc=" ".join(f[:-4]), n=n, total_ms=total_ms, mean_us=mean_us, tflops=tfl, wino=line.startswith("winoG "), wino4=line.startswith("wino4G "),
                        f44="F(4,4)" in line)
    return best, rep


MFMA_MOPS_FLOP = 512.0               # SQ_INSTS_VALU_MFMA_MOPS_F32 counts fp32 MFMA work in units of 512 FLOP (rocprofv3's MfmaFlopsF32 =
                                     # MOPS_F32 * 512): 8 per v_mfma_f32_32x32x2_f32, 4 per v_mfma_f32_16x16x4_f32 (the WN layers' F(2,5) stream)


def other_configs(net, dev):
    """The other single-GPU configurations of BASELINE.json, timed after the timed region so that every one of them carries a
    driver-run number: C1 1 x 200 (the reference notebook's shape: latency), C3 32 x 512, C5 8 x 4096 (long form).  Same protocol
    as the headline: inputs resident in HBM, 2 untimed calls (the second captures the replay plan where the shape qualifies),
    then K back-to-back `infer` calls between HIP events on the launch stream."""
    from cases import sw
    out = {}
    for tag, B, T, K in (("c1_1x200", 1, 200, 20), ("c3_32x512", 32, 512, 5), ("c5_8x4096", 8, 4096, 4), ("b4_4x512", 4, 512, 10)):
        mel = torch.from_numpy(sw.synthetic_mel(1000 + len(out), B, T)).to(dev)
        eps = torch.from_numpy(sw.synthetic_eps(1000 + len(out), B, T)).to(dev)
        ln = torch.full((B,), T, dtype=torch.int64, device=dev)
        with torch.no_grad():
            for _ in range(3):
                o = net.infer(mel, ln, noise_scale=0.667, eps=eps)[0]
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(K):
                o = net.infer(mel, ln, noise_scale=0.667, eps=eps)[0]
            e1.record()
            torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / K
        n = o.numel()
        out[tag] = {"ms_per_step": ms, "samples_per_s": n / (ms * 1e-3), "real_time_factor": n / (ms * 1e-3) / SAMPLE_RATE, "steps": K,
                    "finite": bool(torch.isfinite(o).all())}
        del mel, eps, o
    out["note"] = ("SynthesizerTrn.infer, synthetic mels, full lengths; c3 is the batch-32 configuration (the reference's infer takes no "
                   "speaker embedding: models.py:331-339; the g-conditioned modules are covered by the parity tests); b4_4x512 is a mid-size "
                   "serving batch (VERDICT r5 item 4), not a BASELINE configuration")
    return out


def live_hbm_traffic(B, T, timeout_s=150):
    """Three child runs of this script under `rocprofv3 --pmc` on the DEFAULT launch plan (read-request counters, write-request
    counters, SQ_INSTS_VALU_MFMA_MOPS_F32: separate passes, no tracing beside them), 2 steps each; returns (HBM bytes of the
    GEMM-family kernels per step, description, fp32 MFMA operations per step as the hardware counted them, in units of 512 FLOP).
    The children run with --full minus its other legs: the last two steps of their traces, which are counted, are then the
    dominant-kernel probe's two direct-launch calls."""
    import shutil, subprocess, tempfile
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import pmc_traffic
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(prof):
        raise RuntimeError("rocprofv3 not found")
    env = dict(os.environ, TMPDIR="/tmp")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    base = tempfile.mkdtemp(prefix="svoc_pmc_", dir="/tmp")
    try:
        dirs = []
        for tag, counters in (("rd", pmc_traffic.READ_COUNTERS), ("wr", pmc_traffic.WRITE_COUNTERS), ("mfma", ["SQ_INSTS_VALU_MFMA_MOPS_F32"])):
            d = os.path.join(base, tag)
            cmd = [prof, "--pmc", *counters, "-d", d, "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__),
                   "--steps", "2", "--warmup", "1", "--batch", str(B), "--frames", str(T), "--full", "--no-cpu-baseline", "--no-pmc", "--no-other-configs"]
            r = subprocess.run(cmd, cwd="/tmp", env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=timeout_s)
            if r.returncode != 0:
                raise RuntimeError(f"rocprofv3 pass {tag} exit {r.returncode}: {r.stdout[-200:].decode(errors='replace')}")
            dirs.append(d)
        tj = pmc_traffic.traffic(dirs[0], dirs[1], 0, 2)
        if tj["gemm_family_launches_per_step"] < 1:
            raise RuntimeError("no GEMM-family dispatches in the counter traces")
        mfma = pmc_traffic.counter_per_step(dirs[2], "SQ_INSTS_VALU_MFMA_MOPS_F32", 2)
        return (tj["gemm_family_read_bytes_per_step"] + tj["gemm_family_write_bytes_per_step"],
                f"LIVE: `rocprofv3 --pmc` child runs of bench.py after the timed region ({', '.join(pmc_traffic.READ_COUNTERS)} | "
                f"{', '.join(pmc_traffic.WRITE_COUNTERS)} | SQ_INSTS_VALU_MFMA_MOPS_F32; 2 steps each, {tj['dispatches_counted_per_step']:.0f} dispatches per step; "
                f"whole step {((tj['hbm_read_bytes_per_step'] + tj['hbm_write_bytes_per_step']) / 1e9):.1f} GB)", mfma)
    finally:
        shutil.rmtree(base, ignore_errors=True)


DUMP_BYTES = 64_000_000              # --dump-outputs: the whole dump stays under 64 MB
DUMP_SEED = 1001


def dump_outputs(d, arrays):
    """Write every array of `arrays` ({name: tensor}) as d/<name>.npy in float32.  If together they exceed DUMP_BYTES, each
    keeps the same share of its elements: a seeded sample, flattened, in increasing index order (the same shapes pick the same
    positions in every run).  Returns {name: description} for the JSON line."""
    import zlib
    os.makedirs(d, exist_ok=True)
    total = sum(t.numel() for t in arrays.values())
    budget = (DUMP_BYTES - 4096 * len(arrays)) // 4                 # float32 elements, with room for the .npy headers
    info = {}
    for name, t in arrays.items():
        a = t.detach().to(device="cpu", dtype=torch.float32).contiguous().numpy()
        rec = {"shape": list(a.shape), "dtype": "float32", "sampled": total > budget}
        if total > budget:
            k = budget * a.size // total
            rng = np.random.default_rng([DUMP_SEED, zlib.crc32(name.encode())])
            a = a.reshape(-1)[np.sort(rng.choice(a.size, size=k, replace=False, shuffle=False))]
            rec.update(elements=int(k), sample=f"seeded ({DUMP_SEED}, crc32 of the name) choice of {k} of {t.numel()} flat indices, ascending")
        np.save(os.path.join(d, name + ".npy"), a)
        info[name] = rec
    return info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=16, help="utterances per GPU")
    ap.add_argument("--frames", type=int, default=512, help="mel frames per utterance")
    ap.add_argument("--full", action="store_true", help="after the timed region also run every measurement and check beyond the headline "
                                                          "(dominant kernel, PMC passes, other configs, CPU baseline + parity; N>1: scatter, infer_sharded)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baseline and the parity check against the oracle")
    ap.add_argument("--no-pmc", action="store_true", help="--full: skip the live HBM-traffic passes (rocprofv3 --pmc child runs of this script)")
    ap.add_argument("--no-other-configs", action="store_true", help="--full: skip the C1 / C3 / C5 timings after the timed region")
    ap.add_argument("--allow-no-collective", action="store_true", help="N>1: do not fail when neither gather nor all_gather works")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write the last timed step's outputs as DIR/<name>.npy (float32, <= 64 MB in all)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    import cases
    from cases import sw
    from smart_vocoder_amd import models, parallel, _native

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        if world == 1 and args.gpus > 1:
            raise SystemExit("launch multi-GPU runs with torch.distributed.run (one process per GPU)")
        args.gpus = world
    assert torch.cuda.is_available(), "bench.py needs an MI355X"
    ndev = torch.cuda.device_count()
    dev_index = local_rank % max(1, ndev)          # (a 1-GPU box can still smoke-test the N>1 code path with gloo)
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    dist = None
    cdev = dev                                     # device of the small control tensors of the collectives
    # one process launched by torch.distributed.run (RANK set, WORLD_SIZE 1) still builds its process group and runs the
    # scatter / gather: the RCCL data path executes on a 1-GPU box (tests/test_parallel_gpu.py)
    use_dist = world > 1 or (os.environ.get("BENCH_FORCE_DIST") == "1" and "RANK" in os.environ)
    if use_dist:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        backend = os.environ.get("BENCH_BACKEND", "nccl")          # "nccl" is RCCL on ROCm
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
            cdev = torch.device("cpu")

    B, T = args.batch, args.frames
    sd_np = cases.full_model_weights(skip_enc_q=True, file_cache=False)
    net = models.SynthesizerTrn(513, 32, n_speakers=109, **cases.IITP_MODEL)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd_np.items()}, strict=False)
    net = net.to(dev).eval()

    # Weak scaling: every rank owns a 16x512 shard that is resident in HBM before the timed region.  The job's
    # batch is created on rank 0 and scattered over RCCL/xGMI (setup, untimed); if that collective is unavailable
    # the shard is regenerated locally from the same deterministic generator (identical values).
    Bj = B * world
    mel = eps = ln = None
    scatter_ok = False
    if use_dist:
        try:
            if rank == 0:
                full = [torch.from_numpy(sw.synthetic_mel(1001, Bj, T)).to(dev), torch.full((Bj,), T, dtype=torch.int64, device=dev),
                        torch.from_numpy(sw.synthetic_eps(1001, Bj, T)).to(dev)]
            else:
                full = None
            mel, ln, eps = parallel.scatter_batch(full, [(80, T), (), (192, T)], [torch.float32, torch.int64, torch.float32],
                                                  Bj, src=0, device=dev)
            scatter_ok = True
        except Exception as e:   # noqa: BLE001
            if rank == 0:
                print(f"[bench] scatter failed ({type(e).__name__}: {e}); generating shards locally", file=sys.stderr)
            mel = None
    if mel is None:
        a, b_ = rank * B, (rank + 1) * B
        mel = torch.from_numpy(sw.synthetic_mel(1001, Bj, T)[a:b_]).to(dev)
        eps = torch.from_numpy(sw.synthetic_eps(1001, Bj, T)[a:b_]).to(dev)
        ln = torch.full((B,), T, dtype=torch.int64, device=dev)

    gather_mode = {"v": "gather" if use_dist else "none"}
    gather_out = {"v": None}                       # rank 0's receive buffer [Bj, 1, L]: allocated once, outside the timed region

    def collect(o):
        """waveforms back to rank 0 (inside the timed region): RCCL gather, falling back to all_gather"""
        if gather_mode["v"] == "gather":
            if rank == 0 and gather_out["v"] is None:
                gdev = o.device if cdev.type != "cpu" else torch.device("cpu")
                gather_out["v"] = torch.empty((Bj,) + tuple(o.shape[1:]), dtype=o.dtype, device=gdev)
            return parallel.gather_waveforms(o, Bj, dst=0, out=gather_out["v"])
        if gather_mode["v"] == "all_gather":
            out = torch.empty((Bj,) + tuple(o.shape[1:]), dtype=o.dtype, device=o.device)
            dist.all_gather_into_tensor(out, o.contiguous())
            return out
        return o

    marks = []                                     # N>1: (before infer, after infer, after gather) events of every timed step, on the launch stream
    last = []                                      # infer's outputs of the last timed step (--dump-outputs)

    def step(timed=False, keep=False):
        if timed and use_dist:
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            ev[0].record()
            res = net.infer(mel, ln, noise_scale=0.667, eps=eps)
            ev[1].record()
            r = collect(res[0])
            ev[2].record()
            marks.append(ev)
        else:
            res = net.infer(mel, ln, noise_scale=0.667, eps=eps)
            r = collect(res[0])
        if keep:
            last[:] = [res]
        return r

    if use_dist:   # choose a collective that works on this node before any timing
        with torch.no_grad():
            o_probe = net.infer(mel, ln, noise_scale=0.667, eps=eps)[0]
            for mode in ("gather", "all_gather", "none"):
                gather_mode["v"] = mode
                ok = torch.ones(1, device=cdev)
                try:
                    collect(o_probe)
                    torch.cuda.synchronize()
                except Exception as e:   # noqa: BLE001
                    ok.zero_()
                    print(f"[bench] rank {rank}: {mode} failed ({type(e).__name__}: {e})", file=sys.stderr)
                dist.all_reduce(ok, op=dist.ReduceOp.MIN)
                if ok.item() > 0:
                    break
        if gather_mode["v"] == "none" and not args.allow_no_collective:
            if rank == 0:
                print("[bench] no collective (gather / all_gather) works on this node: the N>1 line would not include the "
                      "waveform gather; refusing (pass --allow-no-collective to run replicas only)", file=sys.stderr)
            dist.destroy_process_group()
            raise SystemExit(3)

    with torch.no_grad():
        for _ in range(args.warmup):
            out = step()
        torch.cuda.synchronize()
        _native.stats_reset()
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        ev0.record()                     # the HIP kernels are enqueued on torch's current stream
        for i in range(args.steps):
            out = step(timed=True, keep=i == args.steps - 1)
        ev1.record()
        torch.cuda.synchronize()
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        # a persistent WN launch of the timed region that gave up a wait made its call's waveform NaN and raised the library's error word: the line is
        # not printed for such a run (include/svoc.h svoc_check_async_error; needs no synchronisation beyond the one above)
        _native.check_async_error()
    gpu_ms = ev0.elapsed_time(ev1)
    dumped = None
    if args.dump_outputs and rank == 0:
        # what a caller of the timed path receives from its last step: infer's outputs (N=1) or the gathered waveforms (N>1)
        o_last, x_mask, (z, z_p, m_p, logs_p) = last[0]
        arrays = {"o": out} if use_dist else {"o": o_last, "x_mask": x_mask, "z": z, "z_p": z_p, "m_p": m_p, "logs_p": logs_p}
        dumped = dump_outputs(args.dump_outputs, arrays)
    last.clear()
    stats = _native.stats_get()
    scatter_ms = None
    if use_dist and scatter_ok and args.full:
        # the other collective of the data path, timed on its own (setup in the weak-scaling protocol, so not inside `value`):
        # rank 0's job batch -> one 16 x T shard per rank, K times, barrier + synchronize on both sides, max over ranks
        full = None
        if rank == 0:
            full = [torch.from_numpy(sw.synthetic_mel(1001, Bj, T)).to(dev), torch.full((Bj,), T, dtype=torch.int64, device=dev),
                    torch.from_numpy(sw.synthetic_eps(1001, Bj, T)).to(dev)]
        nsc = max(1, min(args.steps, 5))
        torch.cuda.synchronize(); dist.barrier(); torch.cuda.synchronize()
        ts = time.perf_counter()
        for _ in range(nsc):
            parallel.scatter_batch(full, [(80, T), (), (192, T)], [torch.float32, torch.int64, torch.float32], Bj, src=0, device=dev)
        torch.cuda.synchronize(); dist.barrier(); torch.cuda.synchronize()
        tsc = torch.tensor([(time.perf_counter() - ts) / nsc * 1e3], dtype=torch.float64, device=cdev)
        dist.all_reduce(tsc, op=dist.ReduceOp.MAX)
        scatter_ms = float(tsc.item())
    per_rank = sharded = None
    if use_dist:
        tt = torch.tensor([dt], dtype=torch.float64, device=cdev)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt_own, dt = dt, float(tt.item())
        # Attribution of the N>1 line: per rank, the mean device time of `infer` and of the waveform gather inside the
        # timed steps (HIP events on the launch stream; the gather's span includes waiting for the slowest peer) and the rank's own wall time.
        inf_ms = sum(e[0].elapsed_time(e[1]) for e in marks) / max(1, len(marks))
        gat_ms = sum(e[1].elapsed_time(e[2]) for e in marks) / max(1, len(marks))
        mine = torch.tensor([dt_own / args.steps * 1e3, inf_ms, gat_ms, gpu_ms / args.steps], dtype=torch.float64, device=cdev)
        allr = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(allr, mine)
        per_rank = {"step_wall_ms": [float(t[0]) for t in allr], "infer_ms": [float(t[1]) for t in allr], "gather_ms": [float(t[2]) for t in allr],
                    "step_gpu_ms": [float(t[3]) for t in allr]}
        if args.full:
            # The public entry point itself: parallel.infer_sharded (ONE scatter of (lengths | mel | eps) from rank 0 + infer + ONE gather per call,
            # shapes passed by the caller so that nothing is broadcast or read back), K calls between the same barriers.  A second figure:
            # `value` stays the weak-scaling step above (inputs resident on every rank), this one moves the job's inputs from rank 0 every call.
            full = None
            if rank == 0:
                full = [torch.from_numpy(sw.synthetic_mel(1001, Bj, T)).to(dev), torch.full((Bj,), T, dtype=torch.int64, device=dev),
                        torch.from_numpy(sw.synthetic_eps(1001, Bj, T)).to(dev)]
            sh_out = None
            if rank == 0:
                sh_out = torch.empty((Bj, 1, T * net.dec.hop), dtype=torch.float32, device=dev if cdev.type != "cpu" else torch.device("cpu"))
            try:
                with torch.no_grad():
                    def sharded_call():
                        return parallel.infer_sharded(net, full[0] if full else None, full[1] if full else None, full[2] if full else None,
                                                      noise_scale=0.667, src=0, shape=(Bj, T), out=sh_out)
                    for _ in range(max(1, min(2, args.warmup))):
                        o_sh = sharded_call()
                    torch.cuda.synchronize(); dist.barrier(); torch.cuda.synchronize()
                    ts = time.perf_counter()
                    for _ in range(args.steps):
                        o_sh = sharded_call()
                    torch.cuda.synchronize(); dist.barrier(); torch.cuda.synchronize()
                tsh = torch.tensor([time.perf_counter() - ts], dtype=torch.float64, device=cdev)
                dist.all_reduce(tsh, op=dist.ReduceOp.MAX)
                sharded = {"ms_per_call": float(tsh.item()) / args.steps * 1e3, "calls": args.steps,
                           "samples_per_s": Bj * T * net.dec.hop * args.steps / float(tsh.item()),
                           "what": "parallel.infer_sharded(shape=(B, T), out=...): scatter of the job's inputs from rank 0 + infer + gather per call, max over ranks"}
                if rank == 0:
                    sharded["equals_timed_step_output"] = bool(torch.equal(o_sh.to(out.device), out))
            except Exception as e:   # noqa: BLE001
                sharded = {"error": f"{type(e).__name__}: {e}"[:300]}
            del full

    if rank == 0:
        samples_per_step = Bj * T * net.dec.hop
        value = samples_per_step * args.steps / dt
        # dominant kernel family: the fp32-MFMA implicit-GEMM kernels (every convolution of the path; ResBlock
        # iterations of the C=32/64 stages and WN layers run as fused kernels of the same family).  Algorithmic FLOPs of the
        # launches in the timed region (counted by the library, 2*MAC) over the device time of the region measured
        # with HIP events on the launch stream (includes the few % spent in the small non-GEMM kernels).
        conv_tflops = stats["conv_flops"] / (gpu_ms * 1e-3) / 1e12
        exec_tflops = stats["executed_flops"] / (gpu_ms * 1e-3) / 1e12
        dom, _ = dominant_kernel_probe(net, mel, ln, eps) if (args.full and B == 16 and T == 512) else (None, None)
        res = {
            "metric": "audio samples/sec (22.05 kHz), iitp_base batch 16 per GPU",
            "value": value, "unit": "samples/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f32", "data": "synthetic",
            "config": {"workload": f"configs/iitp_base.json SynthesizerTrn.infer, {B}x{T}-frame synthetic mels per GPU "
                                   f"(BASELINE.json configs[1]), noise_scale 0.667, random-init trained-like weights",
                       "global_batch": Bj, "frames": T, "samples_per_step": samples_per_step, "parallelism": f"dp{world}", "collective": gather_mode["v"],
                       "scatter_ms": scatter_ms, "scatter_note": "RCCL scatter of (mel, lengths, eps) from rank 0, timed separately after the timed region; the timed step = infer + waveform gather"},
            "real_time_factor": value / SAMPLE_RATE / world,
            "samples_per_s_per_gpu": value / world,
        }
        if dumped is not None:
            res["dump_outputs"] = {"dir": os.path.abspath(args.dump_outputs), "arrays": dumped}
        if per_rank is not None:
            res["per_rank"] = per_rank
            res["step_ms_min_over_ranks"] = min(per_rank["step_wall_ms"])
            res["step_ms_max_over_ranks"] = max(per_rank["step_wall_ms"])
            res["infer_ms_min_over_ranks"], res["infer_ms_max_over_ranks"] = min(per_rank["infer_ms"]), max(per_rank["infer_ms"])
            res["gather_ms"] = per_rank["gather_ms"][0]
            res["per_rank_note"] = ("means over the timed steps; infer_ms / gather_ms = HIP events on each rank's launch stream around net.infer and the "
                                    "waveform gather (rank 0's gather span includes waiting for the slowest peer), step_wall_ms = the rank's own wall clock "
                                    "between the barriers; `ms_per_step` is the max over ranks")
            res["infer_sharded"] = sharded
        res["scaling_curve"] = ("this line is one point of the weak-scaling curve (the driver derives efficiency from the N = 1, 2, 4, 8 lines)" if world > 1 else
                                "NOT MEASURED by this line: world size 1 moves no bytes over xGMI; no scaling number is claimed")
        # Roofline.  `achieved` / `frac` (round 4): 2*MAC the matrix pipe really ISSUED in the timed region - counted per launch by
        # the library (the Winograd kernels issue a fixed share of the direct form's multiply-adds) and checked against the hardware's
        # SQ_INSTS_VALU_MFMA_MOPS_F32 count below - over the device time of the region (HIP events on the launch stream; conservative: the region
        # includes the few % of non-GEMM kernels).  Bounded by the FP32 MFMA peak.  `achieved_direct_form` / `frac_direct_form` price
        # the ALGORITHMIC direct-form FLOPs of SURVEY.md 8(d) (2 568 280 per sample) over the same time: a statement about time to
        # solution that the peak does not bound (Winograd arithmetic does the same convolutions with fewer multiply-adds).
        res["roofline"] = {"bound": "mfma", "achieved": exec_tflops, "peak": FP32_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                           "frac": exec_tflops / FP32_MFMA_PEAK_TFLOPS,
                           "achieved_direct_form": conv_tflops, "frac_direct_form": conv_tflops / FP32_MFMA_PEAK_TFLOPS,
                           "executed_mfma_flop_fraction": stats["executed_flops"] / max(1.0, stats["conv_flops"]),
                           "executed_flop_per_step": stats["executed_flops"] / args.steps,
                           "executed_flops_pmc": None,
                           "winograd_form_floor_ms": stats["executed_flops"] / args.steps / (FP32_MFMA_PEAK_TFLOPS * 1e12) * 1e3,
                           "direct_form_floor_ms": stats["conv_flops"] / args.steps / (FP32_MFMA_PEAK_TFLOPS * 1e12) * 1e3,
                           "traffic": None,
                           "kernel": "fp32 MFMA implicit-GEMM family: conv_wino4(_group|_acc3|_pair)_kernel (every ResBlock convolution of the decoder, all four stages: Winograd F(4,4) for k=7/11, F(4,3) for k=3), convt_wino_kernel (F(4,2), upsamplers), conv_mfma_kernel, wn_layer_fused(_ks)_kernel (fallbacks: resblock_fused_ct_kernel, conv_wino(_group)_kernel F(2,3), conv_group_kernel)",
                           "note": "achieved/frac = executed 2*MAC / time (<= peak). Shares of the direct form's multiply-adds issued per kernel size k=3/7/11: "
                                   "F(4,3) (k=3) 1/2; F(4,4) (k=7/11 in every stage) 3.5/7, 5.25/11 (merged accumulate launch: k=3 1.75/3 too); "
                                   "F(2,3) (fall-back) 2/3, 5/7, 8/11; F(4,2) upsamplers 5/8; F(2,5) WN in_layers 3/5; everything else 1. "
                                   "achieved_direct_form/frac_direct_form = algorithmic direct-form 2*MAC (SURVEY.md 8d) / time, NOT bounded by the peak; "
                                   "winograd_form_floor_ms = executed FLOPs of one step at 157.3 TFLOP/s",
                           "gemm_launches_per_step": stats["conv_launches"] / args.steps,
                           "convolutions_per_step": stats["convolutions"] / args.steps,
                           "small_kernel_launches_per_step": stats["other_launches"] / args.steps,
                           "flop_per_step": stats["conv_flops"] / args.steps,
                           "gpu_ms_per_step_rank0": gpu_ms / args.steps}
        if dom:
            # the launch with the largest share of the step.  achieved / frac = the multiply-adds its MFMAs really executed
            # ((5.25 + 3.5 + 1.5) / (11 + 7 + 3) of the direct form with k=11/7 in F(4,4); (6.5 + 4 + 1.5) / 21 in F(4,3); F(2,3):
            # (8 + 5 + 2) / 21) over its launch time
            executed = (10.25 / 21.0 if dom["f44"] else 12.0 / 21.0) if dom["wino4"] else (15.0 / 21.0 if dom["wino"] else 1.0)
            res["roofline"]["dominant_kernel"] = {
                "name": (("conv_wino4_group_kernel<1,4,0,true> " if dom["f44"] else "conv_wino4_group_kernel<1,4> ") if dom["wino4"] else
                         ("conv_wino_group_kernel<1,4> " if dom["wino"] else "conv_group_kernel<2,2,2,2> ")) + dom["desc"],
                "launches_measured": dom["n"], "avg_launch_us": dom["mean_us"],
                "flop_per_launch_direct_form": dom["tflops"] * 1e12 * dom["mean_us"] * 1e-6,
                "flop_per_launch": dom["tflops"] * 1e12 * dom["mean_us"] * 1e-6 * executed,
                "achieved": dom["tflops"] * executed, "frac": dom["tflops"] * executed / FP32_MFMA_PEAK_TFLOPS,
                "achieved_direct_form": dom["tflops"], "frac_direct_form": dom["tflops"] / FP32_MFMA_PEAK_TFLOPS,
                "executed_mfma_flop_fraction": executed,
                "measured": "hipEventRecord around every launch on the launch stream (library event profiler), after the timed region"}
        # HBM traffic of the same workload from PMC counters (--full).  They cannot be read from inside this process: at N=1 two child runs
        # of this script (2 steps, no CPU leg) are made under `rocprofv3 --pmc`, read- and write-request counters in separate
        # passes as MI355X_MICROARCH.md prescribes, and summed per step by tools/pmc_traffic.py.  If the profiler is missing, fails
        # or times out, the figure is taken from this round's committed passes instead and labelled OFFLINE.
        step_bytes, tsrc, mfma_insts = None, None, None
        under_profiler = any(k.startswith(("ROCPROF", "ROCP_TOOL")) for k in os.environ)      # never nest profilers
        if args.full and world == 1 and not args.no_pmc and not under_profiler and B == 16 and T == 512:
            try:
                step_bytes, tsrc, mfma_insts = live_hbm_traffic(B, T)
            except Exception as e:   # noqa: BLE001
                res["roofline"]["traffic_live_error"] = f"{type(e).__name__}: {e}"[:300]
        if args.full and step_bytes is None:
            import glob
            tfiles = sorted(glob.glob(os.path.join(ROOT, "profiles", f"{ROUND_TAG}*_pmc_hbm_traffic.json")))
            if tfiles and B == 16 and T == 512:
                try:
                    tj = json.load(open(tfiles[-1]))
                    step_bytes = tj["gemm_family_read_bytes_per_step"] + tj["gemm_family_write_bytes_per_step"]
                    tsrc = f"OFFLINE: profiles/{os.path.basename(tfiles[-1])} (rocprofv3 --pmc TCC_EA0_RDREQ_*/WRREQ_*, separate passes)"
                except Exception:   # noqa: BLE001
                    pass
        if mfma_insts is not None:
            # hardware check of the library's bookkeeping: SQ_INSTS_VALU_MFMA_MOPS_F32 of one step of the DEFAULT plan x 512 FLOP
            # (includes the padding of ragged tiles, which the library's counter leaves out)
            res["roofline"]["executed_flops_pmc"] = mfma_insts * MFMA_MOPS_FLOP
            res["roofline"]["executed_flops_pmc_over_library"] = mfma_insts * MFMA_MOPS_FLOP / max(1.0, stats["executed_flops"] / args.steps)
            res["roofline"]["frac_pmc"] = mfma_insts * MFMA_MOPS_FLOP / (gpu_ms / args.steps * 1e-3) / 1e12 / FP32_MFMA_PEAK_TFLOPS
        if step_bytes is not None:
            res["roofline"]["traffic"] = step_bytes / max(1.0, res["roofline"]["gemm_launches_per_step"])
            res["roofline"]["traffic_unit"] = "HBM bytes per GEMM-family launch (mean over gemm_launches_per_step)"
            res["roofline"]["traffic_bytes_per_step"] = step_bytes
            res["roofline"]["traffic_source"] = tsrc
        if args.full and world == 1 and B == 16 and T == 512 and not args.no_other_configs and not under_profiler:
            try:
                res["other_configs"] = other_configs(net, dev)
            except Exception as e:   # noqa: BLE001
                res["other_configs"] = {"error": f"{type(e).__name__}: {e}"[:300]}
        fail = None
        if args.full and world == 1 and not args.no_cpu_baseline:
            keep = {}
            res["cpu_baseline"] = cpu_baseline(sd_np, 1001, keep)
            if B == 16 and T == 512 and "c2" in keep:
                # parity of the timed configuration itself: the GPU waveform of the last timed step against the oracle's
                # waveform of the same mel / eps (seed 1001), whole batch (north_star: RMS <= 1e-3; relative RMS <= 1e-4)
                ref = keep["c2"].double()
                err = out.detach().cpu().double() - ref
                rms, ref_rms = float(err.pow(2).mean().sqrt()), float(ref.pow(2).mean().sqrt())
                res["parity"] = {"rms": rms, "rel_rms": rms / ref_rms, "max_abs": float(err.abs().max()), "ref_rms": ref_rms,
                                 "against": "oracle/vocoder_oracle.py (CPU fp32) on the bench batch, 16x512, seed 1001, all 2 097 152 samples",
                                 "tolerance": {"rms": 1e-3, "rel_rms": 1e-4}}
                if not (rms <= 1e-3 and rms / ref_rms <= 1e-4):
                    fail = f"parity of the timed configuration failed: rms {rms:.3e}, rel {rms / ref_rms:.3e}"
        print(json.dumps(res))
        if fail:
            print("[bench] " + fail, file=sys.stderr)
            raise SystemExit(4)
    if use_dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
