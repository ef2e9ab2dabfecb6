"""The WN conformance bounds (cases.WN_REL_RMS = R, cases.WN_MAX_ERR = A; tests/test_gpu_wn_forms.py) against the legitimate numerics of
the GPU forms and against a small defect of the gate, emulated in the oracle on the CPU at a 4-layer H = 192, k = 5 stack on 1 x 512
(every other operation in float64).  No GPU needed.

  emulation                                                     rel-RMS     max|err| / rms(ref)   vs R = 2e-6
  in_layer in Winograd F(2,5) (points 0, +-1, +-2, inf), fp32     8.5e-7        5.0e-6             below R / 2: admitted
  tanh half of the gate scaled by (1 + 1e-5)                     9.3e-6        4.3e-5             above 2 R: refused

The F(2,5) figure is the fp32 error the GPU's default layer form adds on top of float64 by construction (transforms, products and the
sum over the 192 channels all in fp32); the gate defect is ten times smaller than the 1e-4 relative slack of the per-module parity bound
(tests/test_gpu_parity.py check()), which it passes."""
import contextlib
from fractions import Fraction

import numpy as np
import torch

import cases
from cases import sw
from oracle import vocoder_oracle as O

H, K, NL, B, T = 192, 5, 4, 1, 512
SEED = 12500


def cook_toom(m, r, pts):
    """(AT m x n, G n x r, BT n x n) of the correlation F(m, r) at the points `pts` and infinity, exactly in fractions, as float64
    (the construction of tools/wino_numerics.py)."""
    n = m + r - 1

    def vander(cols):
        return [[Fraction(p) ** j for j in range(cols)] for p in pts] + [[Fraction(0)] * (cols - 1) + [Fraction(1)]]

    A, G = vander(m), vander(r)
    for i, p in enumerate(pts):
        d = Fraction(1)
        for j, q in enumerate(pts):
            if i != j:
                d *= Fraction(p) - Fraction(q)
        G[i] = [g / d for g in G[i]]

    def times(c, q):     # coefficients of c(x) * (x - q)
        return [(c[k - 1] if k > 0 else Fraction(0)) - Fraction(q) * (c[k] if k < len(c) else Fraction(0)) for k in range(len(c) + 1)]

    BT = []
    for i in range(len(pts)):
        c = [Fraction(1)]
        for j, q in enumerate(pts):
            if i != j:
                c = times(c, q)
        BT.append(c + [Fraction(0)] * (n - len(c)))
    c = [Fraction(1)]
    for q in pts:
        c = times(c, q)
    BT.append(c)
    f = lambda M: np.array([[float(x) for x in row] for row in M])
    return f(A).T, f(G), f(BT)


AT, G, BT = cook_toom(2, 5, [0, 1, -1, 2, -2])


def f25_conv_fp32(w, b, x):
    """'same' k = 5 convolution of x [1, C, T] with w [Co, C, 5] in F(2,5) form: weight and input transforms, the six products summed
    over the channels and the output transform, all in float32; + bias."""
    w32, x32 = w.numpy().astype(np.float32), x[0].numpy().astype(np.float32)
    C, Tn = x32.shape
    nw = (Tn + 1) // 2
    xp = np.zeros((C, 2 * nw + 4), np.float32)
    xp[:, 2:2 + Tn] = x32
    d = np.stack([xp[:, 2 * q:2 * q + 6] for q in range(nw)], 1)                     # [C, windows, 6]
    V = np.einsum("cqj,ij->icq", d, BT.astype(np.float32)).astype(np.float32)       # [6, C, windows]
    U = np.einsum("ock,ik->ioc", w32, G.astype(np.float32)).astype(np.float32)      # [6, Co, C]
    M = np.matmul(U, V).astype(np.float32)                                           # [6, Co, windows], fp32 sums over C
    y = np.einsum("mi,ioq->oqm", AT.astype(np.float32), M).astype(np.float32).reshape(w32.shape[0], 2 * nw)[:, :Tn]
    y = torch.from_numpy(y).double()[None]
    return y if b is None else y + b.double()[None, :, None]


@contextlib.contextmanager
def patched(in_layer_f25=False, tanh_scale=None):
    conv, gate = O._conv, O.gate

    def conv_f25(sd, prefix, x, dilation=1, padding=0, groups=1):
        if ".in_layers." not in "." + prefix or dilation != 1:
            return conv(sd, prefix, x, dilation=dilation, padding=padding, groups=groups)
        return f25_conv_fp32(O.conv_weight(sd, prefix).double(), O._bias(sd, prefix), x)

    def gate_scaled(a, g, h):
        s = a + g
        return torch.tanh(s[:, :h]) * tanh_scale * torch.sigmoid(s[:, h:])

    if in_layer_f25:
        O._conv = conv_f25
    if tanh_scale is not None:
        O.gate = gate_scaled
    try:
        yield
    finally:
        O._conv, O.gate = conv, gate


def error(**kw):
    sd = {k: torch.from_numpy(v).double() for k, v in sw.fill_state_dict(cases.wn_shapes(H, K, NL, 0), SEED).items()}
    x = torch.from_numpy(cases.rnd(SEED, "x", (B, H, T), 1.0)).double()
    mask = torch.ones(B, 1, T, dtype=torch.float64)
    args = dict(hidden=H, kernel_size=K, dilation_rate=1, n_layers=NL)
    with torch.no_grad():
        ref = O.wn(sd, "", x, mask, None, **args).numpy()
        with patched(**kw):
            emu = O.wn(sd, "", x, mask, None, **args).numpy()
    rr = float(np.sqrt((ref ** 2).mean()))
    return float(np.sqrt(((emu - ref) ** 2).mean())) / rr, float(np.abs(emu - ref).max()) / rr


def test_f25_transforms_are_exact():
    """The F(2,5) matrices in float64 reproduce the direct correlation to rounding."""
    rng = np.random.default_rng(0)
    d, g = rng.standard_normal((1000, 6)), rng.standard_normal((1000, 5))
    direct = np.stack([(d[:, i:i + 5] * g).sum(1) for i in range(2)], 1)
    assert np.abs(((g @ G.T) * (d @ BT.T)) @ AT.T - direct).max() < 1e-12


def test_fp32_f25_in_layer_is_within_the_wn_bound():
    rel, mx = error(in_layer_f25=True)
    assert 1e-8 < rel <= cases.WN_REL_RMS / 2 and mx <= cases.WN_MAX_ERR / 2, (rel, mx)


def test_gate_defect_of_1e5_exceeds_the_wn_bound():
    rel, mx = error(tanh_scale=1 + 1e-5)
    assert rel >= 2 * cases.WN_REL_RMS, f"rel-RMS {rel:.2e} is within 2x of the bound {cases.WN_REL_RMS:.1e}"
