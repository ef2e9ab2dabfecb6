"""The MRF conformance bounds (cases.MRF_REL_RMS = R, tests/test_gpu_mrf_forms.py) against reduced-precision operand streams in the
ResBlock convolutions alone, emulated in the oracle on the CPU: activation and weight split into bf16 hi + lo words and the partial
products summed in float64, at a C = 64 and a C = 32 shape of the GPU matrix with one row.  No GPU needed.

  stream                                 C = 64 (T 1000)   C = 32 (T 4082)   vs R = 3.5e-6
  hi*hi + hi*lo + lo*hi (lo*lo dropped)      4.7e-6            1.6e-6        at the fp32 level: the bound cannot refuse it
  hi*hi + hi*lo (the lo*hi term dropped)     1.8e-3            5.9e-4        > 100 R: refused

So the bound refuses a split stream that loses one of its cross terms, and operands staged through fp16 (the fp16 control in the GPU
file, ~1e-4), but a complete three-term split-bf16 stream lands within the fp32 kernels' own spread (1.7e-6 worst at C = 256) and
passes: the lo*lo term and the residues beyond two bf16 words weigh ~2^-17 of a product."""
import contextlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cases
from oracle import vocoder_oracle as O


@contextlib.contextmanager
def split_bf16_oracle(terms):
    """O._conv with a split-bf16 stream for the ResBlock convolutions (prefixes containing 'resblocks.'): the sum of the partial
    products named in `terms` ("hh", "hl" = x_hi * w_lo, "lh" = x_lo * w_hi), in float64."""
    orig = O._conv

    def bf(t):
        return t.to(torch.bfloat16).to(torch.float64)

    def conv(sd, prefix, x, dilation=1, padding=0, groups=1):
        if "resblocks." not in prefix:
            return orig(sd, prefix, x, dilation=dilation, padding=padding, groups=groups)
        w = O.conv_weight(sd, prefix).to(torch.float64)
        b = O._bias(sd, prefix)
        x = x.to(torch.float64)
        xh, wh = bf(x), bf(w)
        part = {"hh": (xh, wh), "hl": (xh, bf(w - wh)), "lh": (bf(x - xh), wh)}
        y = sum(F.conv1d(part[t][0], part[t][1], None, dilation=dilation, padding=padding, groups=groups) for t in terms)
        return y if b is None else y + b.to(torch.float64)[None, :, None]

    O._conv = conv
    try:
        yield
    finally:
        O._conv = orig


def stream_error(C, Tn, terms):
    c, sd = cases.mrf_stage_weights(C)
    sd = {k: torch.from_numpy(v).double() for k, v in sd.items()}
    x = torch.from_numpy(cases.mrf_stage_input(C, 1, Tn)).double()
    kw = dict(prefix="", resblock="1", resblock_kernel_sizes=c["rks"], resblock_dilation_sizes=c["rds"], upsample_rates=c["ur"],
              upsample_kernel_sizes=c["uks"])
    with torch.no_grad():
        ref = O.generator(sd, x, **kw).numpy()
        with split_bf16_oracle(terms):
            emu = O.generator(sd, x, **kw).numpy()
    assert (np.abs(ref) > 0.99).mean() <= 0.05
    return float(np.sqrt(((emu - ref) ** 2).mean() / (ref ** 2).mean()))


@pytest.mark.parametrize("C,Tn", [(64, 1000), (32, 4082)])
def test_split_bf16_stream_missing_a_cross_term_exceeds_the_mrf_bound(C, Tn):
    rel = stream_error(C, Tn, ("hh", "hl"))
    assert rel >= 2 * cases.MRF_REL_RMS, f"C = {C}: rel-RMS {rel:.2e} is within 2x of the bound {cases.MRF_REL_RMS:.1e}"


@pytest.mark.parametrize("C,Tn", [(64, 1000), (32, 4082)])
def test_split_bf16_three_term_stream_error(C, Tn):
    """The complete three-term stream is an fp32-level stream (see the table above): its error is the emulation's and must be
    nonzero and far below the cross-term case; a regression of the emulation itself would show here."""
    rel3 = stream_error(C, Tn, ("hh", "hl", "lh"))
    rel2 = stream_error(C, Tn, ("hh", "hl"))
    assert 1e-7 < rel3 < 1e-5 and rel2 > 50 * rel3, (rel3, rel2)
