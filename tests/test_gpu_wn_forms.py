"""Form-by-form conformance of the gated WaveNet stack (WN: the mel encoder's 16 layers, the couplings' 8) against a float64 oracle.

Each case runs one modules.WN on its own under the event profiler, so every row of the report belongs to the WN, asserts the exact
multiset of launch forms that ran, and compares rows 0, B/2, B - 1 of the output (for a grouped stack launch also the last row of
group 0 and the first of group 1) with oracle.vocoder_oracle.wn run on float64 copies of the weights, input, mask and g.  Only each
row's valid columns are measured.  Bounds (cases.WN_REL_RMS = R, cases.WN_MAX_ERR = A): rel-RMS <= R and max|err| <= A * rms(ref).
The whole output must be finite, and every column at or past an utterance's length exactly 0 (the reference returns out * mask).

Forms (csrc/engine.hip WNStack::forward; a form is the profiler row with its N and B dropped):
  meshWN   the whole stack in one persistent launch for short inputs, 1 or 2 tiles per group (csrc/wn_mesh.hip; unconditioned only)
  smallWN  one launch per layer for short inputs, one or two row pairs per workgroup (pp2), + the last 1 x 1 as a conv (csrc/wn_small.hip)
  stackWN  the whole stack in one persistent launch, once per group of whole utterances beyond its capacity (csrc/wn_stack.hip)
  fusedWN  one launch per layer (csrc/wn_fused.hip): F(2,5) at H = 192 k = 5 d = 1, else the direct form (ksplit, NA32 / NA64)
  conv     the in_layer with the gate epilogue (m2) and the 1 x 1 res_skip as two convolutions per layer; the cond_layer
  g1 / gT  on smallWN / fusedWN: conditioned by g of one frame / of T frames.
A tile is 32 columns; tiles = B * ceil(T / 32).  Gates at 256 CUs: short below 96 tiles (3/8 of the CUs); the mesh launch takes up to
10 groups of 1 or 2 tiles; smallWN pp2 at 43 .. 85 tiles; the stack holds one tile per CU.  Every case took the form the gates predict
on the MI355X; the small chain's last 1 x 1 and the two-convolution path run as K-split convolutions.  A shard of one utterance under
variant_batch(B) may take another form than the whole job: wn_stack_applies counts the shard's own tiles, so a row of 17 x 512 (per-layer
F(2,5), 17 does not split into groups) runs the stack launch.  That is safe because the stack's arithmetic is the per-layer kernel's
instruction for instruction, and test_wn_shard_equals_whole_job pins it bit for bit.

Measured against float64 on the MI355X (worst compared row; rel-RMS, max|err| / rms(ref)):
  meshWN 1 / 2 tiles per group       4.6e-7 .. 4.9e-7   2.0e-6 .. 2.5e-6
  smallWN pp1 / pp2, + g1 / gT       3.8e-7 .. 4.5e-7   2.0e-6 .. 2.4e-6
  stackWN x 1 / x 2 / x 4            6.8e-7 .. 7.1e-7   3.8e-6 .. 4.4e-6   (16 layers: 7.1e-7, the worst)
  fusedWN F(2,5), + g1 / gT          5.5e-7 .. 6.8e-7   3.3e-6 .. 3.9e-6
  fusedWN direct: ksplit CT (SVOC_WN_F25=0) 4.3e-7 .. 4.5e-7; ksplit H64 2.4e-7; NA64 2.9e-7; NA32 H160 4.2e-7; two convs 2.5e-7
  R = 2e-6, A = 2e-5.  R is 2.8x the worst form rather than 2x: tests/test_wn_bounds_cpu.py must admit the fp32 F(2,5) in_layer
  emulated on the CPU (8.5e-7) at R / 2.  No form stands out: the F(2,5) forms sit at 1.1 .. 1.6x the direct form of the same shape.
Mutations (built aside, not kept): the gate's sigmoid scaled by (1 + 1e-5) in the stack and mesh kernels measures 9.6e-6 .. 1.0e-5 on
every stack and mesh case and fails them (tests/test_gpu_parity.py catches the stack half only, through its bitwise comparison with the
per-layer launches, and passes the mesh half); one F(2,5) output-transform coefficient off by 1e-5 measures 1.8e-5 .. 2.6e-5 on every
F(2,5) case and fails them (tests/test_gpu_parity.py passes it).
"""
import collections
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import cases
from cases import sw
from oracle import vocoder_oracle as O

pytestmark = pytest.mark.gpu

R, A = cases.WN_REL_RMS, cases.WN_MAX_ERR
WN_KINDS = ("meshWN", "smallWN", "stackWN", "fusedWN")


def T_(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def forms(*parts):
    c = collections.Counter()
    for p in parts:
        c.update(p)
    return c


def mesh(NL, NT):
    return {f"meshWN H192 k5 d1 {NL} layers, one launch ({NT} tile{'s' if NT > 1 else ''} per group), F(2,5)": 1}


def stack(NL, n=1):
    return {f"stackWN H192 k5 d1 {NL} layers, one launch, F(2,5)": n}


def cond(gin, NL, H=192):
    return {f"conv Ci{gin} Co{2 * H * NL} k1 d1 m0": 1}


def small(NL, pp2=False, g="", gin=0):
    """The short-input chain: layer 0, layers 1 .. NL - 1 with the previous layer's res_skip at their head, the last res_skip as a conv."""
    m = (" pp2" if pp2 else "") + (" " + g if g else "")
    return forms({f"smallWN H192 k5 d1 F(2,5){m}": 1}, {f"smallWN H192 k5 d1 F(2,5) + res_skip{m}": NL - 1}, {"conv Ci192 Co192 k1 d1 ksplit m0": 1},
                 cond(gin, NL) if g else {})


def fused(NL, H=192, k=5, dr=1, variant="NA32 ksplit F(2,5)", g=""):
    m = " " + g if g else ""
    c = collections.Counter()
    for i in range(NL):
        c[f"fusedWN H{H} k{k} d{dr ** i} {variant}{' last' if i == NL - 1 else ''}{m}"] += 1
    return c


# name -> (H, k, dr, NL, gin, B, T, g frames or None, expected forms)
CASES = {
    "mesh1_c1":      (192, 5, 1, 16, 0, 1, 200, None, mesh(16, 1)),
    "mesh1_ragged":  (192, 5, 1, 8, 0, 10, 30, None, mesh(8, 1)),
    "mesh2_odd":     (192, 5, 1, 8, 0, 2, 288, None, mesh(8, 2)),
    "mesh2_max":     (192, 5, 1, 16, 0, 1, 640, None, mesh(16, 2)),
    "small1":        (192, 5, 1, 8, 0, 1, 700, None, small(8)),
    "small1_hi":     (192, 5, 1, 8, 0, 1, 3000, None, small(8)),
    "small2_lo":     (192, 5, 1, 8, 0, 1, 1376, None, small(8, True)),
    "small2_hi":     (192, 5, 1, 16, 0, 5, 540, None, small(16, True)),
    "stack_lo":      (192, 5, 1, 8, 0, 6, 512, None, stack(8)),
    "stack_c2":      (192, 5, 1, 16, 0, 16, 512, None, stack(16)),
    "stack_tail":    (192, 5, 1, 8, 0, 8, 520, None, stack(8)),
    "groups2":       (192, 5, 1, 8, 0, 32, 512, None, stack(8, 2)),
    "groups_c5":     (192, 5, 1, 16, 0, 8, 4096, None, stack(16, 4)),
    "fused_odd":     (192, 5, 1, 8, 0, 17, 512, None, fused(8)),
    "fused_tail":    (192, 5, 1, 8, 0, 16, 520, None, fused(8)),
    "cond_small_g1": (192, 5, 1, 8, 256, 1, 200, 1, small(8, False, "g1", 256)),
    "cond_pp2_gT":   (192, 5, 1, 8, 16, 4, 512, "T", small(8, True, "gT", 16)),
    "cond_fused_c3": (192, 5, 1, 8, 256, 32, 512, 1, forms(fused(8, g="g1"), cond(256, 8))),
    "cond_fused_gT": (192, 5, 1, 8, 16, 8, 1024, "T", forms(fused(8, g="gT"), cond(16, 8))),
    "direct_ks":     (64, 3, 2, 3, 16, 8, 2048, 1, forms(fused(3, 64, 3, 2, "NA32 ksplit", "g1"), cond(16, 3, 64))),
    "direct_nr2":    (64, 3, 2, 3, 0, 16, 2048, None, fused(3, 64, 3, 2, "NA64")),
    "direct_nr1":    (160, 3, 1, 2, 0, 4, 1024, None, fused(2, 160, 3, 1, "NA32")),
    "two_conv":      (96, 5, 1, 2, 0, 1, 100, None, {"conv Ci96 Co192 k5 d1 ksplit m2": 2, "conv Ci96 Co192 k1 d1 ksplit m0": 1,
                                                                   "conv Ci96 Co96 k1 d1 ksplit m0": 1}),
}


def wn_forms(report):
    """Multiset of the WN launch forms in an svoc_profile_report: rows of the WN kinds and conv rows, each description with its N and B
    (and a conv's tile shape) dropped and its blanks collapsed, counted by the n column."""
    out = collections.Counter()
    for line in report.splitlines():
        t = line.split()
        if len(t) < 5 or t[0] not in WN_KINDS + ("conv",):
            continue
        desc = [x for x in t[:-4] if not re.fullmatch(r"[NB]\d+|\d+x\d+x\d+x\d+", x)]
        out[" ".join(desc)] += int(t[-4])
    return out


def unlayered(form):
    """A form without its layer count (the persistent launches name it): the path's stacks have other depths than the cases'."""
    return re.sub(r" \d+ layers,", " layers,", form)


@pytest.fixture(scope="module")
def N():
    from smart_vocoder_amd import _native
    assert torch.cuda.is_available()
    _native.lib()
    return _native


_MODULES = {}


def module(H, k, dr, NL, gin):
    """(WN on the GPU, float64 state dict) for one configuration, made once."""
    key = (H, k, dr, NL, gin)
    if key not in _MODULES:
        from smart_vocoder_amd import modules
        sd = sw.fill_state_dict(cases.wn_shapes(H, k, NL, gin), 12600 + H + 10 * k + 100 * dr + NL + gin)
        m = modules.WN(H, k, dr, NL, gin_channels=gin)
        m.load_state_dict({n: T_(v) for n, v in sd.items()})
        _MODULES[key] = (m.cuda().eval(), {n: T_(v).double() for n, v in sd.items()})
    return _MODULES[key]


def lengths_of(B, Tn):
    """Row 0 full length, the last row ending inside a tile, one utterance of length 1 where B >= 3, the rest in [T/2, T]."""
    rng = np.random.default_rng(B * 10000 + Tn)
    lens = [Tn] + [int(rng.integers(Tn // 2, Tn + 1)) for _ in range(B - 1)]
    if B >= 2:
        lens[-1] = Tn - 13 if Tn % 32 != 13 else Tn - 14
    if B >= 3:
        lens[1] = 1
    return lens


class Inputs:
    def __init__(self, name, seed=0, B=None, Tn=None, scale=1.0):
        H, k, dr, NL, gin, B0, T0, gT, _ = CASES[name]
        B, Tn = B or B0, Tn or T0
        s = 12700 + seed + sum(map(ord, name))
        self.lens = lengths_of(B, Tn)
        self.mask = T_(cases.lengths_mask(self.lens, Tn))
        self.x = T_(cases.rnd(s, "x", (B, H, Tn), scale)) * self.mask
        self.g = None if gT is None else T_(cases.rnd(s, "g", (B, gin, 1 if gT == 1 else Tn), 1.0))


def run(N, name, inp, profile=True):
    """(output on the CPU, WN forms) of one forward of the case's module."""
    H, k, dr, NL, gin = CASES[name][:5]
    m, _ = module(H, k, dr, NL, gin)
    N.profile_enable(profile)
    try:
        with torch.no_grad():
            y = m(inp.x.cuda(), inp.mask.cuda(), g=None if inp.g is None else inp.g.cuda())
        torch.cuda.synchronize()
        rep = N.profile_report() if profile else ""
    finally:
        N.profile_enable(False)
    return y.cpu(), wn_forms(rep)


def compared_rows(name, B):
    rows = {0, B // 2, B - 1}
    n = sum(v for k, v in CASES[name][8].items() if k.startswith("stackWN"))
    if n > 1:                   # the grouped stack launch: the rows on either side of the first group boundary
        rows |= {B // n - 1, B // n}
    return sorted(rows)


def errors(name, y, inp, rows=None):
    """Worst (rel-RMS, max|err| / rms(ref)) over the compared rows' valid columns against float64, after the checks on the whole output:
    finite, and exactly 0 at and past every utterance's length."""
    H, k, dr, NL, gin = CASES[name][:5]
    _, sd64 = module(H, k, dr, NL, gin)
    assert torch.isfinite(y).all(), f"{name}: non-finite output"
    for b, n in enumerate(inp.lens):
        assert not y[b, :, n:].any(), f"{name}: row {b} is nonzero past its length {n}"
    rows = compared_rows(name, y.shape[0]) if rows is None else rows
    with torch.no_grad():
        ref = O.wn(sd64, "", inp.x[rows].double(), inp.mask[rows].double(), None if inp.g is None else inp.g[rows].double(),
                   hidden=H, kernel_size=k, dilation_rate=dr, n_layers=NL).numpy()
    rel = mx = 0.0
    for i, b in enumerate(rows):
        n = inp.lens[b]
        r, e = ref[i, :, :n], y[b, :, :n].double().numpy() - ref[i, :, :n]
        rr = float(np.sqrt((r ** 2).mean()))
        rel, mx = max(rel, float(np.sqrt((e ** 2).mean())) / rr), max(mx, float(np.abs(e).max()) / rr)
    return rel, mx


def assert_bounds(name, rel, mx):
    print(f"WN-FIGURES {name}: rel-RMS {rel:.3e} max|err|/rms(ref) {mx:.3e}")
    assert rel <= R and mx <= A, f"{name}: rel-RMS {rel:.3e} (bound {R:.1e}), max|err|/rms(ref) {mx:.3e} (bound {A:.1e})"


def switches_set():
    return any(k.startswith("SVOC_") and k not in ("SVOC_LIB", "SVOC_VARIANT_JOBS") for k in os.environ)


def show(f):
    return sorted(f.items())


# ----------------------------------------------------------------------------- the matrix
@pytest.mark.parametrize("name", list(CASES))
def test_wn_form_vs_float64(N, name):
    """One case of the matrix: the exact multiset of WN forms, and the compared rows within R / A of float64."""
    inp = Inputs(name)
    y, f = run(N, name, inp)
    print(f"WN-FORMS {name}: {show(f)}")
    if not switches_set():      # (a variant run may take other kernels)
        assert f == CASES[name][8], f"{name}: WN forms\n  ran      {show(f)}\n  expected {show(CASES[name][8])}"
    assert_bounds(name, *errors(name, y, inp))


# name -> (B, T) of an unrelated call of the same module that takes the same family of launch forms at another shape
STALE_CASES = {"mesh1_c1": (1, 300), "mesh2_odd": (1, 600), "small2_lo": (2, 700), "stack_lo": (5, 700), "groups2": (16, 1024),
               "fused_odd": (9, 1000)}


@pytest.mark.parametrize("name", list(STALE_CASES))
def test_wn_ignores_earlier_calls(N, name):
    """Nothing of an earlier call may reach a later one: the persistent launches exchange tile edges and hand-over rows through device
    memory and the chains ping-pong through a workspace.  x, then an unrelated call with its input scaled by 1e3, then x again: the same
    bits.  Then x2 = x + 1e-3 * noise right after x and right after the unrelated call: the same bits, and within R / A of float64.  An
    edge left by x has almost the right value for x2, so only this comparison exposes it."""
    inp = Inputs(name)
    Bo, To = STALE_CASES[name]
    other = Inputs(name, seed=7, B=Bo, Tn=To, scale=1e3)
    x2 = Inputs(name)
    x2.x = (inp.x + 1e-3 * T_(cases.rnd(12800 + sum(map(ord, name)), "noise", tuple(inp.x.shape), 1.0))) * inp.mask
    y1, _ = run(N, name, inp, False)
    run(N, name, other, False)
    again, _ = run(N, name, inp, False)
    assert torch.equal(again, y1), f"{name}: the result depends on an earlier call of another shape"
    y2a, _ = run(N, name, x2, False)
    run(N, name, other, False)
    y2b, _ = run(N, name, x2, False)
    assert torch.equal(y2a, y2b), f"{name}: x2 right after x differs from x2 right after an unrelated call"
    assert_bounds(name + " x2", *errors(name, y2a, x2))


# name -> the forms a single row takes under variant_batch(B)
SHARD_CASES = {
    "groups2": stack(8),           # (the whole job: two groups of 16)
    "fused_odd": stack(8),         # wn_stack_applies counts the shard's own tiles: the stack launch, where the whole job runs per layer
    "stack_c2": stack(16),
    "small2_hi": small(16, True),
    "mesh2_odd": mesh(8, 2),
    "cond_fused_c3": forms(fused(8, g="g1"), cond(256, 8)),
}


@pytest.mark.parametrize("name", list(SHARD_CASES))
def test_wn_shard_equals_whole_job(N, name):
    """A shard of one utterance under variant_batch(B) must reproduce that utterance of the whole job bit for bit, whichever form it
    takes (tests/test_parallel_gpu.py relies on it for the whole path)."""
    inp = Inputs(name)
    B = inp.x.shape[0]
    y, f_whole = run(N, name, inp)
    b = B - 1
    one = Inputs(name)
    one.lens, one.mask, one.x = [inp.lens[b]], inp.mask[b:b + 1], inp.x[b:b + 1]
    one.g = None if inp.g is None else inp.g[b:b + 1]
    with N.variant_batch(B):
        ys, f_shard = run(N, name, one)
    print(f"WN-SHARD {name}: whole {show(f_whole)} shard {show(f_shard)}")
    if not switches_set():
        assert f_whole == CASES[name][8], show(f_whole)
        assert f_shard == SHARD_CASES[name], f"{name}: the shard took {show(f_shard)}"
    assert torch.equal(ys[0], y[b]), f"{name}: row {b} alone under variant_batch({B}) differs from the whole job's (max {(ys[0] - y[b]).abs().max():.3e})"


DIRECT_CT = {"stack_c2": 16, "stack_lo": 8}     # case -> layers: 16 x 512 and 6 x 512 with SVOC_WN_F25=0


@pytest.mark.parametrize("name", list(DIRECT_CT))
def test_wn_direct_form_ct_kernel(N, name, tmp_path):
    """The H = 192 K-split direct-form kernel (wn_layer_fused_ks_kernel<true, *>) runs only with SVOC_WN_F25=0, which the process reads
    once: a child process runs the case with it and saves its output and profile report; its rows within R / A of float64, and every
    layer as fusedWN ksplit without F(2,5).  (Neither persistent launch applies without F(2,5).)"""
    NL = DIRECT_CT[name]
    code = f"""
import sys, numpy as np, torch
sys.path.insert(0, {cases.ROOT!r}); sys.path.insert(0, {os.path.join(cases.ROOT, 'tests')!r})
import test_gpu_wn_forms as W
from smart_vocoder_amd import _native
inp = W.Inputs({name!r})
m = W.module(*W.CASES[{name!r}][:5])[0]
_native.profile_enable(True)
with torch.no_grad():
    y = m(inp.x.cuda(), inp.mask.cuda())
torch.cuda.synchronize()
open({str(tmp_path / 'report.txt')!r}, 'w').write(_native.profile_report())
_native.profile_enable(False)
np.save({str(tmp_path / 'y.npy')!r}, y.cpu().numpy())
"""
    env = dict(os.environ, SVOC_WN_F25="0")
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=cases.ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    f = wn_forms(open(tmp_path / "report.txt").read())
    print(f"WN-FORMS {name} SVOC_WN_F25=0: {show(f)}")
    assert f == fused(NL, variant="NA32 ksplit"), show(f)
    y = torch.from_numpy(np.load(tmp_path / "y.npy"))
    assert_bounds(name + " direct form", *errors(name, y, Inputs(name)))


def profiled(N, fn):
    N.profile_enable(True)
    try:
        with torch.no_grad():
            fn()
        torch.cuda.synchronize()
        return N.profile_report()
    finally:
        N.profile_enable(False)


def test_path_wn_forms_are_all_pinned(N):
    """Every WN form that SynthesizerTrn.infer launches at 1 x 200 and 16 x 512, and ResidualCouplingBlock(g) reverse at 32 x 512 with
    g [32, 256, 1], must be one that a case above compares with float64 (layer counts aside).  A change that adds or reroutes a WN form
    fails here until it adds a case for it."""
    from smart_vocoder_amd import models
    net = models.SynthesizerTrn(513, 32, n_speakers=109, **cases.IITP_MODEL)
    sd = cases.full_model_weights(skip_enc_q=True)
    net.load_state_dict({k: T_(v) for k, v in sd.items()}, strict=False)
    net = net.cuda().eval()
    ran = collections.Counter()
    for Bn, Tn in ((1, 200), (16, 512)):
        mel = T_(sw.synthetic_mel(1001, Bn, Tn)).cuda()
        eps = T_(sw.synthetic_eps(1001, Bn, Tn)).cuda()
        ln = torch.full((Bn,), Tn, dtype=torch.int64).cuda()
        ran.update(wn_forms(profiled(N, lambda: net.infer(mel, ln, noise_scale=0.667, eps=eps))))
    flow = models.ResidualCouplingBlock(192, 192, 5, 1, 8, gin_channels=256)
    flow.load_state_dict({k[len("flow."):]: T_(v) for k, v in sd.items() if k.startswith("flow.")})
    flow = flow.cuda().eval()
    z = T_(cases.rnd(12900, "z", (32, 192, 512), 1.0)).cuda()
    g = T_(cases.rnd(12900, "g", (32, 256, 1), 1.0)).cuda()
    ran.update(wn_forms(profiled(N, lambda: flow(z, torch.ones(32, 1, 512).cuda(), g=g, reverse=True))))
    ran = {unlayered(k) for k in ran if k.split()[0] in WN_KINDS}
    print(f"WN-PATH forms: {sorted(ran)}")
    pinned = {unlayered(k) for c in CASES.values() for k in c[8]}
    assert ran, "no WN form in the reports"
    if not switches_set():
        assert ran <= pinned, f"WN forms of the path that no case pins: {sorted(ran - pinned)}"
