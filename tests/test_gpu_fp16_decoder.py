"""The decoder's opt-in fp16 mode (decoder_precision="fp16", csrc/conv_f16.hip) on the GPU.

References: the CPU oracle with every ResBlock convolution emulating the mode's numerics - the activated input and the folded weight
rounded to fp16 (round to nearest even), products summed in float64 - and, for the size of the mode's effect, the plain fp32 oracle
and the reference's own fixtures."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cases
from cases import sw
from oracle import vocoder_oracle as O

pytestmark = pytest.mark.gpu


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


@contextlib.contextmanager
def fp16_oracle(acc=torch.float64):
    """O._conv with the fp16 mode's numerics for the decoder's ResBlock convolutions (prefixes containing 'resblocks.'): input and
    folded weight rounded to fp16, products summed in `acc`."""
    orig = O._conv

    def conv(sd, prefix, x, dilation=1, padding=0, groups=1):
        if "resblocks." not in prefix:
            return orig(sd, prefix, x, dilation=dilation, padding=padding, groups=groups)
        w = O.conv_weight(sd, prefix).half().to(acc)
        b = O._bias(sd, prefix)
        y = F.conv1d(x.half().to(acc), w, b.to(acc) if b is not None else None, dilation=dilation, padding=padding, groups=groups)
        return y.float()

    O._conv = conv
    try:
        yield
    finally:
        O._conv = orig


def emulated(run):
    """(float64-summed emulation, its distance to the float32-summed emulation).

    Every ResBlock convolution rounds its input to fp16, so a difference in summation order anywhere upstream flips roundings
    downstream, and the flips compound along the 6 (ResBlock1) or 2 (ResBlock2) chained convolutions of a chain and over the
    stages: two emulations that differ only in summation precision land 1.8e-5 (gen_small_rb2) to 1.7e-4 (gen_small_g) apart in
    waveform rel-RMS.  The GPU result has to be as close to the float64 emulation as that second emulation, within a factor of 2
    (+ 2e-5); a fixed 5e-5 cannot be met by any summation order but the oracle's own."""
    with fp16_oracle(torch.float64):
        r64 = run()
    with fp16_oracle(torch.float32):
        r32 = run()
    return r64, rel_rms(r32, r64)


def f16_launches(report):
    """Launches of conv_f16.hip in an svoc_profile_report (the n column of its 'convh ... f16' rows)."""
    n = 0
    for line in report.splitlines():
        t = line.split()
        if t and t[0] == "convh":
            n += int(t[t.index("f16") + 1])
    return n


def rel_rms(a, b):
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    return float(np.sqrt(((a - b) ** 2).mean()) / np.sqrt((b ** 2).mean()))


@pytest.fixture(scope="module")
def N():
    from smart_vocoder_amd import _native
    assert torch.cuda.is_available()
    _native.lib()
    return _native


@pytest.fixture(scope="module")
def net(N):
    from smart_vocoder_amd import models
    n = models.SynthesizerTrn(513, 32, n_speakers=109, **cases.IITP_MODEL)
    sd = cases.full_model_weights(skip_enc_q=True)
    missing = n.load_state_dict({k: T(v) for k, v in sd.items()}, strict=False)
    assert all(k.startswith("enc_q.") for k in missing.missing_keys)
    return n.cuda().eval()


@pytest.fixture(scope="module")
def sd():
    return {k: T(v) for k, v in cases.full_model_weights(skip_enc_q=True).items()}


# ----------------------------------------------------------------------------- kernel
SHAPES = [(C, k, d) for C in (256, 128, 64, 32) for k in (3, 7, 11) for d in (1, 3, 5)] + [(96, 7, 3), (96, 11, 1)]


@pytest.mark.parametrize("C,k,d", SHAPES)
def test_conv1d_f16_kernel(N, C, k, d):
    lib = N.lib()
    seed = 300 + C + 7 * k + d
    w = T(cases.rnd(seed, "w", (C, C, k), 1.0 / np.sqrt(C * k)))
    bias = T(cases.rnd(seed, "b", (C,), 0.1))
    w16 = w.half().double()
    wc, bc = w.cuda(), bias.cuda()
    for L, B in ((1, 1), (37, 3), (1000, 1), (4100, 3)):
        if C >= 128 and L == 4100:
            B = 1                                          # keeps the CPU float64 references affordable
        x = T(cases.rnd(seed + L, "x", (B, C, L), 1.0))
        xc = x.cuda()
        for slope, res in ((0.1, True), (1.0, False)):
            a = torch.where(x < 0, x * slope, x) if slope != 1.0 else x
            ref = F.conv1d(a.half().double(), w16, bias.double(), dilation=d, padding=(k * d - d) // 2)
            ref32 = F.conv1d(a.double(), w.double(), bias.double(), dilation=d, padding=(k * d - d) // 2)
            if res:
                ref = ref + x.double(); ref32 = ref32 + x.double()
            y = torch.full((B, C, L), float("nan"), device="cuda")
            N.check(lib.svoc_conv1d_f16(N.stream_ptr(), N.ptr(xc), N.ptr(wc), None, N.ptr(bc), N.ptr(xc) if res else None, N.ptr(y),
                                        B, C, C, L, k, d, ctypes.c_float(slope)))
            got = y.cpu().double()
            assert torch.isfinite(got).all()
            err = (got - ref).abs()
            bound = 2e-5 + 1e-5 * ref.abs()
            assert bool((err <= bound).all()), f"C{C} k{k} d{d} L{L} B{B} slope{slope} res{res}: max|err| {float(err.max()):.3e}"
            # negative control: the kernel's result is the fp16 computation, not an fp32 one
            e16 = float(((got - ref) ** 2).mean().sqrt()); e32 = float(((got - ref32) ** 2).mean().sqrt())
            assert e16 < e32, (C, k, d, L, B, e16, e32)


def test_conv1d_f16_odd_channels_and_refusal(N):
    """Channel counts that are not multiples of 32 (the small Generators' C = 16 stages) and Cin != Cout; even k is refused."""
    lib = N.lib()
    for ci, co, k, d, L in ((16, 16, 5, 3, 33), (48, 80, 3, 1, 70)):
        w = T(cases.rnd(ci + co, "w", (co, ci, k), 1.0 / np.sqrt(ci * k))); bias = T(cases.rnd(ci + co, "b", (co,), 0.1))
        x = T(cases.rnd(ci + co, "x", (2, ci, L), 1.0))
        ref = F.conv1d(torch.where(x < 0, x * 0.1, x).half().double(), w.half().double(), bias.double(), dilation=d, padding=(k * d - d) // 2)
        y = torch.full((2, co, L), float("nan"), device="cuda")
        xc, wc, bc = x.cuda(), w.cuda(), bias.cuda()
        N.check(lib.svoc_conv1d_f16(N.stream_ptr(), N.ptr(xc), N.ptr(wc), None, N.ptr(bc), None, N.ptr(y), 2, ci, co, L, k, d,
                                    ctypes.c_float(0.1)))
        assert float((y.cpu().double() - ref).abs().max()) <= 2e-5 + 1e-5 * float(ref.abs().max())
    x = torch.zeros(1, 32, 16, device="cuda"); w = torch.zeros(32, 32, 4, device="cuda"); y = torch.zeros(1, 32, 16, device="cuda")
    assert lib.svoc_conv1d_f16(N.stream_ptr(), N.ptr(x), N.ptr(w), None, None, None, N.ptr(y), 1, 32, 32, 16, 4, 1, ctypes.c_float(0.1)) == -5


# ----------------------------------------------------------------------------- whole path
@pytest.mark.parametrize("name", ["c1", "ragged", "odd"])
def test_infer_fp16(net, sd, name):
    c = cases.INFER_CASES[name]
    mel, ln, eps = cases.infer_inputs(name)
    o = net.infer(T(mel).cuda(), T(ln).cuda(), noise_scale=c["noise_scale"], max_len=c["max_len"], eps=T(eps).cuda(),
                  decoder_precision="fp16")[0].cpu().numpy()
    gold = cases.golden("infer_" + name)["o"]
    r = rel_rms(o, gold)
    assert 1e-5 <= r <= 1e-3, r
    ref, spread = emulated(lambda: O.infer(sd, T(mel), T(ln), T(eps), c["noise_scale"], c["max_len"])[0].numpy())
    r16 = rel_rms(o, ref)
    print(f"{name}: fp16 vs reference fixture rel-RMS {r:.2e}, vs fp16-emulated oracle {r16:.2e} (emulation spread {spread:.2e})")
    assert r16 <= 2 * spread + 2e-5, (r16, spread)
    assert r16 < r, (r16, r)                               # nearer to the fp16 emulation than to the fp32 reference


def test_infer_fp16_full_size(N, net, sd):
    """The bench batch (16 x 512) against the reference's own fixture, and one utterance of it against the fp16-emulated oracle."""
    c = cases.REF_LARGE_CASES["c2_16x512"]
    mel, ln, eps = cases.large_inputs("c2_16x512")
    o, _, (z, z_p, m_p, logs_p) = net.infer(T(mel).cuda(), T(ln).cuda(), noise_scale=c["noise_scale"], eps=T(eps).cuda(),
                                            decoder_precision="fp16")
    o = o.cpu().numpy()
    d = cases.large_digest(c, o, z.cpu().numpy(), z_p.cpu().numpy(), m_p.cpu().numpy(), logs_p.cpu().numpy())
    r = rel_rms(d["o_sub"], cases.golden("ref_c2_16x512")["o_sub"])
    assert 1e-5 <= r <= 1e-3, r
    ref, spread = emulated(lambda: O.infer(sd, T(mel[15:16]), T(ln[15:16]), T(eps[15:16]), c["noise_scale"])[0].numpy())
    r16 = rel_rms(o[15:16], ref)
    print(f"c2_16x512: fp16 vs reference fixture rel-RMS {r:.2e}; utterance 15 vs fp16-emulated oracle {r16:.2e} (spread {spread:.2e})")
    assert r16 <= 2 * spread + 2e-5, (r16, spread)
    assert r16 < r, (r16, r)


@pytest.mark.parametrize("name", ["gen_small_rb2", "gen_small_g"])
def test_generator_fp16(N, name):
    from smart_vocoder_amd import models
    c = cases.GENERATOR_CASES[name]
    sd_np = sw.fill_state_dict(cases.generator_shapes(c), c["seed"], 1.0)
    m = models.Generator(c["initial_channel"], c["resblock"], c["rks"], c["rds"], c["ur"], c["uic"], c["uks"], gin_channels=c["gin"])
    m.load_state_dict({k: T(v) for k, v in sd_np.items()})
    m = m.cuda().eval()
    x = T(cases.rnd(c["seed"], "x", (c["B"], c["initial_channel"], c["T"]), 1.0))
    g = T(cases.rnd(c["seed"], "g", (c["B"], c["gin"], 1), 1.0)) if c["gin"] else None
    y = m(x.cuda(), g=g.cuda() if g is not None else None, decoder_precision="fp16").cpu().numpy()
    r = rel_rms(y, cases.golden(name)["y"])
    assert 1e-5 <= r <= 1e-3, r
    kw = dict(prefix="", resblock=c["resblock"], resblock_kernel_sizes=c["rks"], resblock_dilation_sizes=c["rds"], upsample_rates=c["ur"],
              upsample_kernel_sizes=c["uks"])
    ref, spread = emulated(lambda: O.generator({k: T(v) for k, v in sd_np.items()}, x, g, **kw).numpy())
    r16 = rel_rms(y, ref)
    assert r16 <= 2 * spread + 2e-5, (r16, spread)
    assert r16 < r, (r16, r)
    # and back: the fp32 mode of the same handle is the golden result again
    y32 = m(x.cuda(), g=g.cuda() if g is not None else None).cpu().numpy()
    assert np.abs(y32 - cases.golden(name)["y"]).max() <= 5e-5 + 1e-4 * np.abs(cases.golden(name)["y"]).max()


# ----------------------------------------------------------------------------- the fp32 mode is untouched; fp16 is deterministic
def test_fp32_unchanged_and_fp16_repeatable(N, net):
    mel, ln, eps = cases.infer_inputs("ragged")
    args = (T(mel).cuda(), T(ln).cuda())
    kw = dict(noise_scale=0.667, eps=T(eps).cuda())
    run = lambda p: [net.infer(*args, **kw, decoder_precision=p)[0].cpu() for _ in range(3)]     # third call replays a captured plan
    a32 = run("fp32")
    a16 = run("fp16")
    b32 = run("fp32")
    for t in a32[1:] + b32:
        assert torch.equal(t, a32[0])
    for t in a16[1:]:
        assert torch.equal(t, a16[0])
    assert not torch.equal(a16[0], a32[0])


def test_fp16_batch_rows_bitwise(N, net):
    Bn, Tn = 4, 200
    mel = T(sw.synthetic_mel(91, Bn, Tn)).cuda(); eps = T(sw.synthetic_eps(91, Bn, Tn)).cuda()
    ln = torch.full((Bn,), Tn, dtype=torch.int64).cuda()
    with N.variant_batch(Bn):
        full = net.infer(mel, ln, noise_scale=0.667, eps=eps, decoder_precision="fp16")[0].cpu()
        for i in range(Bn):
            one = net.infer(mel[i:i + 1], ln[i:i + 1], noise_scale=0.667, eps=eps[i:i + 1], decoder_precision="fp16")[0].cpu()
            assert torch.equal(one[0], full[i]), i


def test_fp16_rebuilt_handle_reapplies_mode(N, net):
    """A weight change rebuilds the handle (in fp32); the Python side must switch the new handle to fp16 again."""
    mel, ln, eps = cases.infer_inputs("odd")
    args = (T(mel).cuda(), T(ln).cuda())
    o16 = net.infer(*args, noise_scale=0.0, eps=T(eps).cuda(), decoder_precision="fp16")[0].cpu()
    net.invalidate()
    o16b = net.infer(*args, noise_scale=0.0, eps=T(eps).cuda(), decoder_precision="fp16")[0].cpu()
    assert torch.equal(o16, o16b)


def test_fp16_stats_count_launches(N, net):
    mel, ln, eps = cases.infer_inputs("odd")
    args = (T(mel).cuda(), T(ln).cuda())
    N.profile_enable(True)                                 # direct launches (no plan replay)
    try:
        N.stats_reset()
        net.infer(*args, noise_scale=0.0, eps=T(eps).cuda(), decoder_precision="fp16")
        torch.cuda.synchronize()
        st = N.stats_get()
        rep = N.profile_report()
    finally:
        N.profile_enable(False)
    # every ResBlock convolution on conv_f16.hip: 4 stages x 3 ResBlock1 x 3 iterations x 2 convolutions, one launch each, all counted
    assert f16_launches(rep) == 72, rep
    assert st["convolutions"] >= 72 and st["conv_launches"] >= 72


# ----------------------------------------------------------------------------- pass-through
def test_chunked_and_stream_fp16(N, net, monkeypatch):
    """Every infer that infer_chunked and stream() issue runs the fp16 decoder (counted launches of conv_f16.hip: 72 per call, and
    none in fp32 mode), and the pieces agree with one-shot fp16 infer.  The agreement bound alone cannot tell the modes apart: the
    chunks' encoder / flow launches pick other fp32 variants (<= 1e-5 apart, test_stream.py), the fp16 roundings downstream amplify
    that (see emulated()) to 1.4e-4 max-abs measured, while fp16 and fp32 differ by only ~2e-4 max-abs on this input."""
    Bn, Tn = 1, 300
    mel = T(sw.synthetic_mel(93, Bn, Tn)).cuda(); eps = T(sw.synthetic_eps(93, Bn, Tn)).cuda()
    ln = torch.full((Bn,), Tn, dtype=torch.int64).cuda()
    one = net.infer(mel, ln, noise_scale=0.667, eps=eps, decoder_precision="fp16")[0]
    calls = [0]
    orig_infer = net.infer

    def counting_infer(*a, **k):
        calls[0] += 1
        return orig_infer(*a, **k)

    monkeypatch.setattr(net, "infer", counting_infer)

    def launches(fn):
        calls[0] = 0
        N.profile_enable(True)
        try:
            r = fn()
            torch.cuda.synchronize()
            rep = N.profile_report()
        finally:
            N.profile_enable(False)
        return r, f16_launches(rep), calls[0]

    ch, n, c = launches(lambda: net.infer_chunked(mel, ln, chunk_frames=128, noise_scale=0.667, eps=eps, decoder_precision="fp16"))
    assert c == 3 and n == 72 * c, (c, n)
    assert float((ch - one).abs().max()) <= 5e-4

    def run_stream(prec):
        s = net.stream(noise_scale=0.667, decoder_precision=prec)
        out = [s.push(mel[:, :, a:a + 70], eps[:, :, a:a + 70]) for a in range(0, Tn, 70)]
        out.append(s.flush())
        return torch.cat(out, 2)

    st, n, c = launches(lambda: run_stream("fp16"))
    assert c >= 2 and n == 72 * c, (c, n)
    assert st.shape == one.shape and float((st - one).abs().max()) <= 5e-4
    _, n32, c32 = launches(lambda: run_stream("fp32"))
    assert c32 >= 2 and n32 == 0, (c32, n32)
