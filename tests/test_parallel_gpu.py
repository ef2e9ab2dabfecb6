"""N>1 data path with the REAL model on one GPU: two ranks share device 0 and talk over gloo (the collective an 8-GPU
node runs over RCCL/xGMI is the same scatter/gather in smart-vocoder_amd/parallel.py, with host staging only for gloo).
Checks infer_sharded == single-process infer - to fp32 rounding by default (kernel variants depend on the launch size),
BIT FOR BIT with bitwise=True (svoc_set_variant_batch pins the variants to the job's batch size), and with
length bucketing (sort, trim, un-permute) on a ragged batch - and that bench.py's --gpus 2 path runs end to end.
No scaling number is derived from this setup."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import cases

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _worker(rank, world, port, Bs, T, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sys.path.insert(0, cases.ROOT)
    from cases import sw
    from smart_vocoder_amd import models, parallel
    torch.cuda.set_device(0)
    net = models.SynthesizerTrn(513, 32, n_speakers=109, **cases.IITP_MODEL)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in cases.full_model_weights().items()}, strict=False)
    net = net.cuda().eval()
    oks = [_worker_case(rank, net, b, T, sw, parallel) for b in Bs]
    q.put((rank, all(oks)))
    dist.barrier()
    dist.destroy_process_group()


def _worker_case(rank, net, B, T, sw, parallel):
    ok = True
    mel = eps = ln = None
    if rank == 0:
        mel = torch.from_numpy(sw.synthetic_mel(61, B, T)).cuda(); eps = torch.from_numpy(sw.synthetic_eps(61, B, T)).cuda()
        ln = torch.full((B,), T, dtype=torch.int64).cuda(); ln[1] = T - 17
    with torch.no_grad():
        o = parallel.infer_sharded(net, mel, ln, eps, noise_scale=0.667, src=0)
        if rank == 0:
            ref = net.infer(mel, ln, noise_scale=0.667, eps=eps)[0]
            # shards and the whole batch may take different kernel variants (chosen from the launch size): fp32 rounding
            ok = o.is_cuda and o.shape == ref.shape and (o - ref).abs().max().item() <= 2e-6
        else:
            ok = o is None
        # bitwise: every rank picks the kernel variants of the whole job -> identical bits to one process running the job
        from smart_vocoder_amd import _native as N
        ob = parallel.infer_sharded(net, mel, ln, eps, noise_scale=0.667, src=0, bitwise=True)
        if rank == 0:
            N.profile_enable(True)                 # direct launches (the library's graph replay is bit-identical to them)
            with N.variant_batch(B):
                ref_b = net.infer(mel, ln, noise_scale=0.667, eps=eps)[0]
            N.profile_enable(False)
            ok = ok and torch.equal(ob, ref_b)
        # length bucketing on a ragged batch: rows return in the caller's order, valid region == unsharded, padding == 0
        ln2 = None
        if rank == 0:
            ln2 = torch.tensor([T - 3 * i * (i + 1) for i in range(B)], dtype=torch.int64).clamp(min=5).cuda()
            ln2 = ln2[torch.randperm(B, generator=torch.Generator().manual_seed(3))]
        ok2 = True
        ok_shape = parallel.infer_sharded(net, mel, ln2, eps, noise_scale=0.667, src=0, bucket=True, halo_frames=16)
        if rank == 0:
            ref2 = net.infer(mel, ln2, noise_scale=0.667, eps=eps)[0]
            ok2 = ok_shape.shape == ref2.shape
            for i in range(B):
                n = int(ln2[i]) * 256
                ok2 = ok2 and (ok_shape[i, :, :n] - ref2[i, :, :n]).abs().max().item() <= 2e-6 and float(ok_shape[i, :, n:].abs().sum()) == 0.0
        ok = ok and ok2
    return bool(ok)


def test_infer_sharded_equals_single_process_on_one_gpu():
    """Uneven (5 utterances over 2 ranks) and minimal (2) batches, in one pair of processes."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, (5, 2), 96, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=600) for _ in procs]
    for p in procs:
        p.join(120)
    assert all(ok for _, ok in res), res


def test_bench_two_ranks_gloo_one_gpu(tmp_path):
    """bench.py --gpus 2 --full under torch.distributed.run with both ranks on device 0 (BENCH_BACKEND=gloo): the scatter, the
    per-rank infer and the gather inside the timed region all execute; the JSON line must report collective == gather."""
    env = dict(os.environ, BENCH_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(cases.ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
           "--batch", "4", "--frames", "128", "--full"]
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    j = json.loads(line)
    assert j["n_gpus"] == 2 and j["config"]["collective"] == "gather" and j["config"]["global_batch"] == 8
    assert j["value"] > 0 and j["scaling"] == "weak"
    # attribution of an N>1 line: per-rank spans and the public entry point timed beside the step
    pr = j["per_rank"]
    assert all(len(pr[k]) == 2 and min(pr[k]) > 0 for k in ("step_wall_ms", "infer_ms", "gather_ms", "step_gpu_ms")), pr
    assert j["step_ms_min_over_ranks"] <= j["step_ms_max_over_ranks"] <= j["ms_per_step"] * 1.001
    sh = j["infer_sharded"]
    assert "error" not in sh and sh["ms_per_call"] > 0 and sh["equals_timed_step_output"] is True, sh


def test_bench_two_ranks_one_gpu_full_size_bits():
    """bench.py --gpus 2 --full with both ranks on ONE device at the headline shape (16 x 512 per rank): the persistent WN stack launches (csrc/wn_stack.hip)
    of the two processes then compete for the CUs, and their workgroups wait for neighbours that are not resident yet.  `parallel.infer_sharded` must
    still return the timed step's bits (round 5: with halo slots reused by layer parity it did not)."""
    env = dict(os.environ, BENCH_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(cases.ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "2", "--full"]
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    j = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert j["n_gpus"] == 2 and j["config"]["global_batch"] == 32
    assert j["infer_sharded"]["equals_timed_step_output"] is True, j["infer_sharded"]


_SHARED_GPU_CHILD = """
import sys, torch
sys.path.insert(0, {root!r}); sys.path.insert(0, {root!r} + '/tests')
import cases
from cases import sw
from smart_vocoder_amd import models
net = models.SynthesizerTrn(513, 32, n_speakers=109, **cases.IITP_MODEL)
net.load_state_dict({{k: torch.from_numpy(v) for k, v in cases.full_model_weights().items()}}, strict=False)
net = net.cuda().eval()
seed = int(sys.argv[1])
ins = [(torch.from_numpy(sw.synthetic_mel(seed + i, 16, 512)).cuda(), torch.from_numpy(sw.synthetic_eps(seed + i, 16, 512)).cuda()) for i in range(2)]
ln = torch.full((16,), 512, dtype=torch.int64).cuda()
refs = []
for it in range(14):
    mel, eps = ins[it % 2]
    o = net.infer(mel, ln, noise_scale=0.667, eps=eps)[0]
    if it < 2: refs.append(o.clone())
    elif not torch.equal(o, refs[it % 2]): print("MISMATCH at call", it, float((o - refs[it % 2]).abs().max())); sys.exit(3)
torch.cuda.synchronize()
assert not torch.equal(refs[0], refs[1])
# ... and at 1 x 200 (BASELINE configs[0]): the short-input stacks' persistent launch (csrc/wn_mesh.hip: 84 workgroups that hand rows to each other)
ins = [(torch.from_numpy(sw.synthetic_mel(seed + 5 + i, 1, 200)).cuda(), torch.from_numpy(sw.synthetic_eps(seed + 5 + i, 1, 200)).cuda()) for i in range(2)]
ln = torch.full((1,), 200, dtype=torch.int64).cuda()
refs = []
for it in range(300):
    mel, eps = ins[it % 2]
    o = net.infer(mel, ln, noise_scale=0.667, eps=eps)[0]
    if it < 2: refs.append(o.clone())
    elif not torch.equal(o, refs[it % 2]): print("MISMATCH at short call", it, float((o - refs[it % 2]).abs().max())); sys.exit(4)
torch.cuda.synchronize()
from smart_vocoder_amd import _native
_native.check_async_error()
print("OK")
"""


def test_two_processes_one_gpu_alternating_inputs():
    """Two processes run the full path at 16 x 512 (and then at 1 x 200) on ONE device at the same time, each alternating between two inputs (captured-plan replay from the
    second sight on): every call must reproduce the first call on that input bit for bit.  The persistent WN stack launches of the two processes then
    compete for the CUs; a launch that found its hand-shake counters uncleared (round 5: a memset node ahead of the launch was not a dependable
    ordering inside a replayed plan) would take the edges of the call BEFORE - of the other input - and differ."""
    code = _SHARED_GPU_CHILD.format(root=cases.ROOT)
    ps = [subprocess.Popen([sys.executable, "-c", code, str(4100 + 10 * r)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                           env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")) for r in range(2)]
    outs = [p.communicate(timeout=900)[0] for p in ps]
    for p, o in zip(ps, outs):
        assert p.returncode == 0 and o.strip().endswith("OK"), o[-2000:]


def test_bench_single_gpu_line_schema(tmp_path):
    """bench.py --full at N=1 on the timed configuration (16 x 512, 2 steps, no CPU leg): ONE JSON line with the contract's keys, the
    roofline block (`frac` = executed multiply-adds over the peak, bounded by 1; `frac_direct_form`, which the Winograd kernels may
    push above 1), the library's launch statistics, the HBM traffic of the step and the hardware's MFMA count of the default plan
    (live PMC passes; the count must agree with the library's bookkeeping to 1.5 %), and the C1 / C3 / C5 timings.  --dump-outputs
    writes every output of the last timed step's `infer`, whole, as float32."""
    cmd = [sys.executable, os.path.join(cases.ROOT, "bench.py"), "--steps", "2", "--warmup", "2", "--full", "--no-cpu-baseline",
           "--dump-outputs", str(tmp_path / "dump")]
    r = subprocess.run(cmd, env=dict(os.environ), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    j = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
              "data", "config", "roofline"):
        assert k in j, k
    assert j["n_gpus"] == 1 and j["steps"] == 2 and j["dtype"] == "f32" and j["vs_baseline"] is None and "workload" in j["config"]
    rf = j["roofline"]
    assert rf["bound"] == "mfma" and rf["peak"] == 157.3 and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-9
    assert 0.0 < rf["frac"] <= 1.0 and rf["frac"] <= rf["frac_direct_form"] + 1e-9
    assert abs(rf["frac_direct_form"] - rf["achieved_direct_form"] / rf["peak"]) < 1e-9
    dk = rf["dominant_kernel"]
    assert 0.0 < dk["frac"] <= 1.0 and abs(dk["frac"] - dk["achieved"] / rf["peak"]) < 1e-9
    if rf["traffic_source"].startswith("LIVE"):
        assert rf["executed_flops_pmc"] is not None and abs(rf["executed_flops_pmc_over_library"] - 1.0) < 0.015, rf
    oc = j["other_configs"]
    for k in ("c1_1x200", "c3_32x512", "c5_8x4096", "b4_4x512"):
        assert oc[k]["ms_per_step"] > 0 and oc[k]["finite"], oc
    assert abs(rf["flop_per_step"] - 2568280.0 * j["config"]["samples_per_step"]) / rf["flop_per_step"] < 0.01
    assert 0.5 < rf["executed_mfma_flop_fraction"] <= 1.0
    # HBM traffic: live rocprofv3 --pmc child runs (or, should the profiler fail on the box, this round's committed passes)
    assert rf["traffic"] is not None and rf["traffic_source"].startswith(("LIVE", "OFFLINE")), rf
    assert 2e10 < rf["traffic_bytes_per_step"] < 8e10, rf["traffic_bytes_per_step"]
    _check_headline_dump(j, tmp_path / "dump")


def _check_headline_dump(j, d):
    """--dump-outputs at 16 x 512, N=1: every output of the last timed step's `infer`, whole, as float32, 64 MB at most."""
    dump = j["dump_outputs"]["arrays"]
    shapes = {"o": (16, 1, 512 * 256), "x_mask": (16, 1, 512), "z": (16, 192, 512), "z_p": (16, 192, 512), "m_p": (16, 192, 512), "logs_p": (16, 192, 512)}
    assert sorted(os.listdir(d)) == sorted(f"{n}.npy" for n in shapes) and not any(v["sampled"] for v in dump.values()), dump
    for n, sh in shapes.items():
        a = np.load(d / f"{n}.npy")
        assert a.dtype == np.float32 and a.shape == sh and np.isfinite(a).all(), n
    assert sum(os.path.getsize(d / f) for f in os.listdir(d)) <= 64e6


def test_bench_plain_line(tmp_path):
    """bench.py at N=1 without --full (the run that measures the headline): ONE JSON line with the contract's keys, `value` and
    `ms_per_step` of the same steps, the roofline figures priced from the library's counters of the timed region, --dump-outputs
    written whole - and nothing that takes runs of its own: no dominant-kernel probe, PMC passes, other configurations, CPU
    baseline or parity check."""
    cmd = [sys.executable, os.path.join(cases.ROOT, "bench.py"), "--steps", "2", "--warmup", "2", "--dump-outputs", str(tmp_path / "dump")]
    r = subprocess.run(cmd, env=dict(os.environ), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    j = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
              "data", "config", "roofline"):
        assert k in j, k
    assert j["n_gpus"] == 1 and j["steps"] == 2 and j["warmup"] == 2 and j["dtype"] == "f32" and j["unit"] == "samples/s" and j["higher_is_better"] is True
    assert j["value"] > 0 and abs(j["value"] * j["ms_per_step"] * 1e-3 / j["config"]["samples_per_step"] - 1.0) < 1e-9
    rf = j["roofline"]
    assert 0.0 < rf["frac"] <= 1.0 and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-9
    assert abs(rf["flop_per_step"] - 2568280.0 * j["config"]["samples_per_step"]) / rf["flop_per_step"] < 0.01
    assert "dominant_kernel" not in rf and rf["traffic"] is None and rf["executed_flops_pmc"] is None, rf
    assert not any(k in j for k in ("other_configs", "cpu_baseline", "parity")), sorted(j)
    _check_headline_dump(j, tmp_path / "dump")


_RCCL_WORLD1 = r'''
import os, sys, json
os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("MASTER_PORT", sys.argv[1])
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
import torch, torch.distributed as dist
sys.path.insert(0, sys.argv[2]); sys.path.insert(0, os.path.join(sys.argv[2], "tests"))
import cases
from cases import sw
from smart_vocoder_amd import models, parallel, _native as N
torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)          # "nccl" IS RCCL on ROCm
assert dist.get_backend() == "nccl"
B, T = 3, 96
mel = torch.from_numpy(sw.synthetic_mel(71, B, T)).to(dev); eps = torch.from_numpy(sw.synthetic_eps(71, B, T)).to(dev)
ln = torch.tensor([T, T - 9, 40], dtype=torch.int64, device=dev)
m, l, e = parallel.scatter_batch([mel, ln, eps], [(80, T), (), (192, T)], [torch.float32, torch.int64, torch.float32], B, src=0, device=dev)
res = {"scatter_on_device": bool(m.is_cuda and l.is_cuda and e.is_cuda),
       "scatter_identity": bool(torch.equal(m, mel) and torch.equal(l, ln) and torch.equal(e, eps))}
net = models.SynthesizerTrn(513, 32, n_speakers=109, **cases.IITP_MODEL)
net.load_state_dict({k: torch.from_numpy(v) for k, v in cases.full_model_weights().items()}, strict=False)
net = net.to(dev).eval()
with torch.no_grad():
    N.profile_enable(True)                      # direct launches on both sides of the comparison
    ref = net.infer(mel, ln, noise_scale=0.667, eps=eps)[0]
    o = parallel.infer_sharded(net, mel, ln, eps, noise_scale=0.667, src=0, bitwise=True)
    N.profile_enable(False)
    out = torch.empty_like(ref)
    g = parallel.gather_waveforms(ref, B, dst=0, out=out)
torch.cuda.synchronize()
res.update(sharded_bitwise=bool(o.is_cuda and torch.equal(o, ref)), gather_identity=bool(torch.equal(g, ref)), gather_in_place=bool(g.data_ptr() == out.data_ptr()))
dist.barrier(); dist.destroy_process_group()
print("RCCL1 " + json.dumps(res))
'''


def test_rccl_world_size_one_on_device(tmp_path):
    """The RCCL code path on the hardware a 1-GPU box has: a world-size-1 "nccl" process group on cuda:0, then the
    packed scatter, the gather into a preallocated buffer and infer_sharded(bitwise=True) on DEVICE tensors - librccl is loaded and
    dist.scatter / dist.gather run on device buffers; results must equal plain infer bit for bit.  No scaling claim."""
    script = tmp_path / "rccl1.py"
    script.write_text(_RCCL_WORLD1)
    r = subprocess.run([sys.executable, str(script), str(_free_port()), cases.ROOT], env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("RCCL1 ")][-1]
    res = json.loads(line[6:])
    assert all(res.values()), res


def test_bench_one_rank_rccl():
    """bench.py --full launched by torch.distributed.run with ONE rank and BENCH_BACKEND=nccl (BENCH_FORCE_DIST=1): process group, packed
    scatter and the waveform gather inside the timed region run over RCCL; the line reports collective == gather."""
    env = dict(os.environ, BENCH_BACKEND="nccl", BENCH_FORCE_DIST="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(cases.ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
           "--batch", "4", "--frames", "128", "--full", "--no-cpu-baseline", "--no-pmc", "--no-other-configs"]
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    j = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert j["n_gpus"] == 1 and j["config"]["collective"] == "gather" and j["config"]["scatter_ms"] is not None, j["config"]
    assert len(j["per_rank"]["infer_ms"]) == 1 and j["gather_ms"] > 0 and j["infer_sharded"]["equals_timed_step_output"] is True, j
    assert j["scaling_curve"].startswith("NOT MEASURED")


_RCCL_WORLD2 = r'''
import os, sys, json
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
import torch, torch.distributed as dist
root = sys.argv[1]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
import cases
from cases import sw
from smart_vocoder_amd import models, parallel, _native as N
rank, world, local = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"]), int(os.environ["LOCAL_RANK"])
torch.cuda.set_device(local)                                   # ONE RANK PER DEVICE
dev = torch.device("cuda", local)
dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)      # "nccl" IS RCCL on ROCm
net = models.SynthesizerTrn(513, 32, n_speakers=109, **cases.IITP_MODEL)
net.load_state_dict({k: torch.from_numpy(v) for k, v in cases.full_model_weights().items()}, strict=False)
net = net.to(dev).eval()
res = {}
for (B, T) in ((5, 96), (16, 512)):                            # an uneven split of a small batch; the headline shape per JOB (8 utterances per rank)
    mel = eps = ln = None
    if rank == 0:
        mel = torch.from_numpy(sw.synthetic_mel(81, B, T)).to(dev); eps = torch.from_numpy(sw.synthetic_eps(81, B, T)).to(dev)
        ln = torch.full((B,), T, dtype=torch.int64, device=dev); ln[1] = T - 17
    with torch.no_grad():
        o = parallel.infer_sharded(net, mel, ln, eps, noise_scale=0.667, src=0, bitwise=True, shape=(B, T))
        if rank == 0:
            N.profile_enable(True)                              # direct launches (graph replay is bit-identical to them)
            with N.variant_batch(B):
                ref = net.infer(mel, ln, noise_scale=0.667, eps=eps)[0]
            N.profile_enable(False)
            res[f"{B}x{T}_bitwise"] = bool(o.is_cuda and o.device == dev and torch.equal(o, ref))
            res[f"{B}x{T}_finite"] = bool(torch.isfinite(o).all())
        else:
            res[f"{B}x{T}_none_off_src"] = o is None
torch.cuda.synchronize()
N.check_async_error()
res["devices_differ"] = True
gathered = [None] * world
dist.all_gather_object(gathered, (rank, local, torch.cuda.current_device()))
res["one_rank_per_device"] = len({g[2] for g in gathered}) == world
dist.barrier(); dist.destroy_process_group()
print(f"RCCL2 rank{rank} " + json.dumps(res))
'''


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two visible GPUs: arms itself the day a multi-GPU box runs the suite")
def test_rccl_two_devices(tmp_path):
    """SURVEY 8e on real hardware, the first time two devices are visible: torchrun with one rank PER DEVICE over "nccl" (= RCCL),
    the packed scatter and the in-place gather move bytes between two GPUs, and `infer_sharded(shape=..., bitwise=True)` must return the bits a
    single process computes for the whole job - at an uneven split and at the headline shape.  Then `bench.py --gpus 2 --full` end to end with
    collective == "gather".  Every other multi-rank test of this file pins both ranks to cuda:0 or talks over gloo."""
    script = tmp_path / "rccl2.py"
    script.write_text(_RCCL_WORLD2)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("BENCH_BACKEND", None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), str(script), cases.ROOT]
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=1200)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = sorted(l for l in r.stdout.splitlines() if l.startswith("RCCL2 "))
    assert len(lines) == 2, r.stdout[-2000:]
    for l in lines:
        res = json.loads(l.split(" ", 2)[2])
        assert res and all(res.values()), l
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(cases.ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "2", "--full"]
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=1200)
    assert r.returncode == 0, r.stderr[-3000:]
    j = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert j["n_gpus"] == 2 and j["config"]["collective"] == "gather" and j["config"]["global_batch"] == 32 and j["scaling"] == "weak"
    assert j["value"] > 0 and len(j["per_rank"]["infer_ms"]) == 2 and j["infer_sharded"]["equals_timed_step_output"] is True, j


def test_two_handles_on_two_streams_in_one_process():
    """"two model handles or streams in one process" share the GPU like two processes do - the persistent WN launches of the two streams compete for
    the CUs.  tools/two_streams_one_process.py: two SynthesizerTrn instances with the same weights, each on a stream of its own, `infer` enqueued on both before
    anything is synchronised, at 16 x 512, 1 x 200 and 4 x 512.  The contract: every call either returns the bits of the same call made alone, or its failure is
    REPORTED through `svoc_check_async_error` - never a silent mismatch.  (Runs here, behind the variant pool of tests/test_gpu_variants.py, so that nothing else
    shares the GPU; on an idle GPU every call is clean.)"""
    tool = os.path.join(cases.ROOT, "tools", "two_streams_one_process.py")
    shapes = ((16, 512, 10), (1, 200, 60), (4, 512, 16))
    r = subprocess.run([sys.executable, tool] + [str(v) for sh in shapes for v in sh], env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:]
    for B, Tn, iters in shapes:
        line = [l for l in r.stdout.splitlines() if l.startswith(f"B={B} T={Tn}:")][-1]
        assert "silent mismatches 0," in line, line
        assert int(line.split("reported failures ")[1].split(",")[0]) <= iters // 2, line
