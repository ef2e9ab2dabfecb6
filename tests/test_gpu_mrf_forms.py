"""Form-by-form conformance of the decoder's multi-receptive-field (MRF) stages against a float64 oracle.

Each case isolates one MRF stage at C = 256 / 128 / 64 / 32 in a one-upsampler Generator (cases.mrf_stage_config: conv_pre 32 -> 2C,
ConvTranspose1d 2C -> C with stride 2, so the stage length is L = 2T, the chains k = 3 / 7 / 11 with dilations 1 / 3 / 5, conv_post),
reads which launch forms ran from the event profiler and compares every sample of three rows of the waveform with the oracle run on
float64 copies of the same weights and input.  Bounds (cases.MRF_REL_RMS = R, cases.MRF_MAX_ERR = A): rel-RMS <= R and
max|err| <= A * rms(ref), about twice the worst fp32 case measured on the MI355X and ten times that.

Forms (csrc/engine.hip Generator::run_mrf_grouped; a form is (profiler kind, C, kernel sizes, dilation, accumulate), N and B dropped):
  wino4G  grouped F(4,3) / F(4,4) step of the three chains; a dilated c1 hands its rows window-major to the c2 behind it
  wino4T  the dilated rows' partial last tile in direct form (wino4_tail_plan), behind its wino4G
  wino4A  the merged accumulate of the three chains' last c2
  wino4P  c1 -> c2 in one launch (C = 64 d = 1; C = 32 d = 1 / 3), and its accumulate form (C = 32, last step)
  winoG   grouped F(2,3) (rows of L % 4 != 0 at d = 1), wino (one convolution in F(2,3) form)
  conv / fusedRB  direct and K-split convolutions on the per-chain streams (the short-input plan, small_stage)

Case matrix (MI355X, 256 CUs, mrf_min_tiles() = 128).  Every size gate is cleared twice over: each case except the tail ones takes the
same forms under variant_batch(B / 2) (the tail plan is a round count and changes with B by design).  Tile widths: F(4,x) columns per
tile 128 at C >= 128 and 256 at C = 64; pair tiles PairGeo::W2 = 240 at C = 64, and 496 / 480 / 468 at C = 32 for d = 1 / 3 / 5.
  case          C    B   T     L     forms (per launch; G = wino4G k11/7/3, A = wino4A, T = wino4T, P = wino4P)
  c256_clean    256  2   1920  3840  G d1 x3, G d3, G d5, A          L a whole number of tiles at d = 1 / 3 / 5
  c256_partial  256  4   1000  2000  same                            partial last column tile (20 / 21 / 20 windows left)
  c256_tail     256  8   1024  2048  same + T d3 + T d5              1 / 3 windows left at d = 3 / 5, dropping them saves a round
  c256_odd      256  4   1001  2002  winoG d1 x3, G d3, G d5, conv k3 / k7 / k11 (the last c2s one by one)
  c128_*        128  4 / 8 / 8 / 8   as at C = 256 (c128_tail: L = 4096, 2 / 1 windows left)
  c64_clean     64   8   1920  3840  P d1, G d3, G d1, G d5, A       pair at d = 1, then grouped
  c64_partial   64   16  1000  2000  same
  c64_tail      64   16  2048  4096  same + T d3 + T d5
  c64_odd       64   16  1001  2002  as c256_odd
  c32_d1_0      32   8   3968  7936  P d1, P d3, P d5 accumulate    L mod 496 = 0
  c32_d1_w2m4   32   8   4214  8428  same                            L mod 496 = 492, L mod 468 = 4
  c32_d3_4      32   8   4082  8164  same                            L mod 480 = 4
  c32_d5_w2m4   32   8   4210  8420  same                            L mod 468 = 464
  c32_odd       32   8   4001  8002  fusedRB k3 / k7 / k11 x d1 / d3 / d5 (short-input plan: C = 32 and L % 4 != 0)
  (test_short_input_plan_and_variant_batch) C = 64, 1 x 1024: fusedRB x 9; under variant_batch(16): the c64 grouped forms
Every grouped launch of these cases has more tiles than CUs, so the persistent workgroups loop over tiles of several batch rows.
Odd T at C >= 64 was expected to run winoG throughout; the profiler shows winoG for the d = 1 steps only.
The dilated c1s keep the F(4,x) kernel (wino4_args refuses L % 4 != 0 at d = 1 only: a dilated window covers 4D columns), and the
last c2s run one by one in direct form (the merged accumulate needs whole windows; single F(2,3) launches need 2 tiles per CU).

Measured against float64 on the MI355X (rel-RMS, max|err| / rms(ref); rows 0, B/2, B-1):
  C = 256  1.43e-6 .. 1.73e-6, max 6.3e-6 .. 7.6e-6   (odd 1.43e-6, tail 1.73e-6)
  C = 128  7.8e-7 .. 9.2e-7,   max 3.6e-6 .. 4.4e-6
  C = 64   9.5e-7 .. 1.14e-6,  max 4.1e-6 .. 5.1e-6   (1 x 1024 short-input plan 7.5e-7; 16 x 1024 1.16e-6)
  C = 32   2.3e-7 .. 2.7e-7,   max 1.7e-6 .. 2.0e-6
  R = 3.5e-6 (2x the worst, C = 256 tail), A = 3.5e-5.  The fp16 decoder (negative control): 3.7e-4 at C = 64, 9.7e-5 at C = 32.
The error grows with C (longer dot products).
"""
import collections
import os
import re

import numpy as np
import pytest
import torch

import cases
from oracle import vocoder_oracle as O

pytestmark = pytest.mark.gpu

R, A = cases.MRF_REL_RMS, cases.MRF_MAX_ERR
MRF_KINDS = ("wino4G", "wino4T", "wino4A", "wino4P", "winoG", "wino", "wino4", "group", "conv", "fusedRB")


def T_(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def F(kind, C, ks, d, acc=False, n=1):
    return {(kind, C, ks, d, acc): n}


def forms(*parts):
    c = collections.Counter()
    for p in parts:
        c.update(p)
    return c


def grouped_steps(C, tail=()):
    """The C >= 128 stage: per dilation a window-major wino4G c1 + wino4G c2, the last c2 as the merged accumulate; `tail`: the
    dilations whose c1 takes the tail launch."""
    return forms(F("wino4G", C, "11/7/3", 1), F("wino4G", C, "11/7/3", 1), F("wino4G", C, "11/7/3", 3), F("wino4G", C, "11/7/3", 1),
                 F("wino4G", C, "11/7/3", 5), F("wino4A", C, "3+7+11", None, True), *[F("wino4T", C, "11/7/3", d) for d in tail])


def pair64(tail=()):
    """C = 64: the d = 1 step as the pair kernel, the d = 3 / 5 steps grouped, the merged accumulate."""
    return forms(F("wino4P", 64, "11/7/3", 1), F("wino4G", 64, "11/7/3", 3), F("wino4G", 64, "11/7/3", 1), F("wino4G", 64, "11/7/3", 5),
                 F("wino4A", 64, "3+7+11", None, True), *[F("wino4T", 64, "11/7/3", d) for d in tail])


def odd(C):
    """L % 4 == 2 at C >= 64: grouped F(2,3) at d = 1, the F(4,x) kernels for the dilated c1s, the last c2s one by one in direct form."""
    return forms(F("winoG", C, "11/7/3", 1, n=3), F("wino4G", C, "11/7/3", 3), F("wino4G", C, "11/7/3", 5),
                 F("conv", C, "3", 1), F("conv", C, "7", 1), F("conv", C, "11", 1))


PAIR32 = forms(F("wino4P", 32, "11/7/3", 1), F("wino4P", 32, "11/7/3", 3), F("wino4P", 32, "11/7/3", 5, True))


def fused(C):
    """The short-input plan: every ResBlock iteration as one fused direct-form launch on its chain's stream."""
    return forms(*[F("fusedRB", C, str(k), d) for k in (3, 7, 11) for d in (1, 3, 5)])


# name -> (C, B, T, expected MRF forms); the stage length is L = 2T
CASES = {
    "c256_clean":   (256, 2, 1920, grouped_steps(256)),
    "c256_partial": (256, 4, 1000, grouped_steps(256)),
    "c256_tail":    (256, 8, 1024, grouped_steps(256, (3, 5))),
    "c256_odd":     (256, 4, 1001, odd(256)),
    "c128_clean":   (128, 4, 1920, grouped_steps(128)),
    "c128_partial": (128, 8, 1000, grouped_steps(128)),
    "c128_tail":    (128, 8, 2048, grouped_steps(128, (3, 5))),
    "c128_odd":     (128, 8, 1001, odd(128)),
    "c64_clean":    (64, 8, 1920, pair64()),
    "c64_partial":  (64, 16, 1000, pair64()),
    "c64_tail":     (64, 16, 2048, pair64((3, 5))),
    "c64_odd":      (64, 16, 1001, odd(64)),
    "c32_d1_0":     (32, 8, 3968, PAIR32),
    "c32_d1_w2m4":  (32, 8, 4214, PAIR32),
    "c32_d3_4":     (32, 8, 4082, PAIR32),
    "c32_d5_w2m4":  (32, 8, 4210, PAIR32),
    "c32_odd":      (32, 8, 4001, fused(32)),
}
OTHER_LAUNCHES = 1            # launches outside the convolution counters besides the tails (conv_post)
SMALL_FORMS = fused(64)       # test_short_input_plan_and_variant_batch: 1 x 1024 at C = 64 ...
SMALL_PINNED_FORMS = pair64() # ... and the same row under variant_batch(16), = a real batch of 16
BENCH_HAS_TAIL = True         # 16 x 512 iitp_base: every dilated step at C >= 64 takes the tail launch

def mrf_forms(report, Cs):
    """Multiset of the MRF launch forms in an svoc_profile_report: rows whose kind is an MRF kernel's and whose input and output
    channel counts are both one of `Cs`, normalised to (kind, C, kernel sizes, dilation or None, accumulate), counted by the n column."""
    out = collections.Counter()
    for line in report.splitlines():
        t = line.split()
        if len(t) < 5 or t[0] not in MRF_KINDS:
            continue
        if t[0] == "fusedRB":
            ci = co = int(t[1][1:])
        else:
            ci, co = int(t[1][2:]), int(t[2][2:])
        if ci != co or ci not in Cs:
            continue
        ks = next(x[1:] for x in t[1:] if re.fullmatch(r"k[0-9/+]+", x))
        m = next((re.fullmatch(r"(?:c1\()?d(\d+)\)?(?:\+c2)?", x) for x in t[1:] if re.fullmatch(r"(?:c1\()?d(\d+)\)?(?:\+c2)?", x)), None)
        out[(t[0], ci, ks, int(m.group(1)) if m else None, "accumulate" in t)] += int(t[-4])
    return out


@pytest.fixture(scope="module")
def N():
    from smart_vocoder_amd import _native
    assert torch.cuda.is_available()
    _native.lib()
    return _native


class Stage:
    """The one-stage Generator at C on the GPU and its float64 oracle."""

    def __init__(self, C):
        from smart_vocoder_amd import models
        self.C = C
        self.c, sd = cases.mrf_stage_weights(C)
        c = self.c
        self.m = models.Generator(c["initial_channel"], c["resblock"], c["rks"], c["rds"], c["ur"], c["uic"], c["uks"], gin_channels=0)
        self.m.load_state_dict({k: T_(v) for k, v in sd.items()})
        self.m = self.m.cuda().eval()
        self.sd64 = {k: T_(v).double() for k, v in sd.items()}

    def run(self, N, x, **kw):
        """(output on the CPU, MRF forms, other_launches) of one forward under the profiler."""
        N.profile_enable(True)
        try:
            N.stats_reset()
            y = self.m(x.cuda(), **kw)
            torch.cuda.synchronize()
            rep = N.profile_report()
            ol = N.stats_get()["other_launches"]
        finally:
            N.profile_enable(False)
        return y.cpu(), mrf_forms(rep, (self.C,)), ol

    def ref(self, x):
        c = self.c
        with torch.no_grad():
            return O.generator(self.sd64, x.double(), prefix="", resblock="1", resblock_kernel_sizes=c["rks"], resblock_dilation_sizes=c["rds"],
                               upsample_rates=c["ur"], upsample_kernel_sizes=c["uks"])


_STAGES = {}
_REFS = {}


def stage(C):
    if C not in _STAGES:
        _STAGES[C] = Stage(C)
    return _STAGES[C]


def case_input(name):
    C, B, Tn, _ = CASES[name]
    return T_(cases.mrf_stage_input(C, B, Tn))


def rows_of(B):
    return sorted({0, B // 2, B - 1})


def errors(name, C, y, x, rows=None):
    """(rel-RMS, max|err| / rms(ref)) of rows of `y` against the float64 oracle (cached per case), after the checks every comparison
    makes: the whole batch finite, tanh not saturated."""
    rows = rows_of(y.shape[0]) if rows is None else rows
    assert torch.isfinite(y).all(), f"{name}: non-finite output"
    key = (name, tuple(rows))
    if key not in _REFS:
        _REFS[key] = stage(C).ref(x[rows]).numpy()
    ref = _REFS[key]
    assert (np.abs(ref) > 0.99).mean() <= 0.05, f"{name}: tanh saturates {(np.abs(ref) > 0.99).mean():.3f} of the reference samples"
    err = y[rows].double().numpy() - ref
    rr = float(np.sqrt((ref ** 2).mean()))
    return float(np.sqrt((err ** 2).mean())) / rr, float(np.abs(err).max()) / rr


def assert_bounds(name, rel, mx):
    assert rel <= R and mx <= A, f"{name}: rel-RMS {rel:.3e} (bound {R:.1e}), max|err|/rms(ref) {mx:.3e} (bound {A:.1e})"


def switches_set():
    return any(k.startswith("SVOC_") and k not in ("SVOC_LIB", "SVOC_VARIANT_JOBS") for k in os.environ)


def tail_launches(f):
    return sum(n for k, n in f.items() if k[0] == "wino4T")


# ----------------------------------------------------------------------------- the matrix
@pytest.mark.parametrize("name", list(CASES))
def test_mrf_form_vs_float64(N, name):
    """One case of the matrix: the exact multiset of MRF forms (a tail launch also counts once in other_launches), and rows 0, B/2,
    B - 1 of the waveform within R / A of float64."""
    C, B, Tn, want = CASES[name]
    x = case_input(name)
    y, f, ol = stage(C).run(N, x)
    if not switches_set():      # (a variant run may take other kernels)
        assert f == want, f"{name}: MRF forms\n  ran      {sorted(f.items(), key=str)}\n  expected {sorted(want.items(), key=str)}"
        assert ol == OTHER_LAUNCHES + tail_launches(want), (name, ol)
    assert_bounds(name, *errors(name, C, y, x))


STALE_CASES = ["c256_partial", "c128_partial", "c64_partial", "c32_d3_4"]


@pytest.mark.parametrize("name", STALE_CASES)
def test_mrf_ignores_stale_workspace(N, name):
    """Nothing zeroes the stage buffers' pad columns between calls: a call at a longer T with its input scaled by 1e3 leaves large
    finite values past the later L in every buffer.  The case shape run behind it must give the same bits as before it (a discarded
    lane may multiply a finite value by zero; a halo read past L may not use it) and stay within the bounds."""
    C, B, Tn, _ = CASES[name]
    st = stage(C)
    x = case_input(name)
    before, _, _ = st.run(N, x)
    xl = T_(cases.mrf_stage_input(C, B, Tn + Tn // 4 + 3, 7) * 1e3)
    yl, _, _ = st.run(N, xl)
    assert torch.isfinite(yl).all()
    after, _, _ = st.run(N, x)
    assert_bounds(name + " behind a longer call", *errors(name, C, after, x))
    assert torch.equal(after, before), f"{name}: the result depends on what an earlier, longer call left in the workspace"


@pytest.mark.parametrize("name", ["c64_partial", "c32_d3_4"])
def test_fp16_decoder_is_outside_the_bound(N, name):
    """Negative control: decoder_precision="fp16" rounds the ResBlock convolutions' operands to 11 bits and nothing else; the same
    comparison must put it at least 5x above R."""
    C, B, Tn, _ = CASES[name]
    x = case_input(name)
    y, _, _ = stage(C).run(N, x, decoder_precision="fp16")
    rel, mx = errors(name, C, y, x)
    assert rel >= 5 * R, f"{name} fp16: rel-RMS {rel:.3e} is within 5x of R = {R:.1e}"


def test_short_input_plan_and_variant_batch(N):
    """1 x 1024 frames at C = 64 (L = 2048) is below mrf_min_tiles(): the short-input plan (per-chain streams).  Under variant_batch(16)
    the same row takes the grouped forms of a real batch of 16 and must equal that batch's row bit for bit; both within the bounds."""
    st = stage(64)
    x = T_(cases.mrf_stage_input(64, 16, 1024, 3))
    full, f_full, _ = st.run(N, x)
    loose, f_loose, _ = st.run(N, x[5:6])
    with N.variant_batch(16):
        pinned, f_pinned, _ = st.run(N, x[5:6])
    if not switches_set():
        assert f_loose == SMALL_FORMS, sorted(f_loose.items(), key=str)
        assert f_full == SMALL_PINNED_FORMS and f_pinned == SMALL_PINNED_FORMS, (sorted(f_full.items(), key=str), sorted(f_pinned.items(), key=str))
    assert torch.equal(pinned, full[5:6])
    assert_bounds("c64 1 x 1024 short-input plan", *errors("c64_small", 64, loose, x[5:6], [0]))
    assert_bounds("c64 16 x 1024", *errors("c64_16x1024", 64, full, x))


def test_bench_shape_forms_are_all_pinned(N):
    """The iitp_base decoder at the benchmark's 16 x 512: every MRF form it launches, (kind, C, dilation, accumulate), tail launches
    included, must be one that a case above compares with float64.  A change that adds or reroutes a form fails here until it adds
    a case for it."""
    from smart_vocoder_amd import models
    from cases import sw
    net = models.SynthesizerTrn(513, 32, n_speakers=109, **cases.IITP_MODEL)
    sd = cases.full_model_weights(skip_enc_q=True)
    net.load_state_dict({k: T_(v) for k, v in sd.items()}, strict=False)
    net = net.cuda().eval()
    mel = T_(sw.synthetic_mel(1001, 16, 512)).cuda()
    eps = T_(sw.synthetic_eps(1001, 16, 512)).cuda()
    ln = torch.full((16,), 512, dtype=torch.int64).cuda()
    N.profile_enable(True)
    try:
        with torch.no_grad():
            net.infer(mel, ln, noise_scale=0.667, eps=eps)
        torch.cuda.synchronize()
        rep = N.profile_report()
    finally:
        N.profile_enable(False)
    ran = {(k[0], k[1], k[3], k[4]) for k in mrf_forms(rep, (256, 128, 64, 32))}
    pinned = {(k[0], k[1], k[3], k[4]) for c in CASES.values() for k in c[3]} | {(k[0], k[1], k[3], k[4]) for k in SMALL_FORMS}
    assert ran, rep
    if not switches_set():
        assert ran <= pinned, f"forms at 16 x 512 that no case pins: {sorted(ran - pinned, key=str)}"
        assert any(k[0] == "wino4T" for k in ran) == BENCH_HAS_TAIL, rep
