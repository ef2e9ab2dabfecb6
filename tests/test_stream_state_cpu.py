"""Stage geometry of the stateful stream (svoc_stream_geometry, include/svoc.h), checked by perturbation on the CPU oracle: for every
stage, changing one input column changes no output farther away than the declared halos, and a change at exactly the declared
distance does change an output (the halos are tight).  No GPU: the library is loaded as test_abi.py loads it."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cases
from cases import sw
from oracle import vocoder_oracle as O


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from smart_vocoder_amd import _native
    return _native


def _synth_config(N, models, resblock, rks, rds, ur, uic, uks, initial_channel=192):
    c = N.svoc_synth_config()
    c.n_mel, c.inter_channels, c.hidden_channels = 80, initial_channel, 192
    c.enc_n_layers, c.enc_kernel_size, c.enc_dilation_rate = 16, 5, 1
    c.flow_n_layers, c.flow_kernel_size, c.flow_dilation_rate, c.flow_n_flows = 8, 5, 1, 4
    c.gin_channels = 0
    c.dec = models._gen_config(initial_channel, resblock, rks, rds, ur, uic, uks, 0)
    return c


def _geometry(built, **kw):
    from smart_vocoder_amd import models
    return models.stream_geometry(_synth_config(built, models, **kw))


IITP = dict(resblock="1", rks=[3, 7, 11], rds=[[1, 3, 5]] * 3, ur=[8, 8, 2, 2], uic=512, uks=[16, 16, 4, 4])


def _f64(sd):
    return {k: torch.from_numpy(np.asarray(v)).double() for k, v in sd.items()}


def _check_reach(fn, x, m0, u, hl, hr, name):
    """fn: input [1, C, L] -> output [1, C', L * u]; perturb input column m0 and compare the changed outputs with
    {n : n - hl <= m0 * u <= n + hr}"""
    with torch.no_grad():
        y0 = fn(x)
        xp = x.clone()
        xp[:, :, m0] += 0.5
        y1 = fn(xp)
    d = (y1 - y0).abs().amax(dim=(0, 1))
    # float64: outputs outside the reach are computed from identical inputs and come out bit-identical; inside it the influence of the
    # column decays geometrically through the WN stacks (down to ~1e-16 at 32 columns), so "changed" means "differs at all"
    changed = torch.nonzero(d > 0).flatten().tolist()
    lo, hi = m0 * u - hr, m0 * u + hl
    assert 0 <= lo and hi < d.numel(), (name, lo, hi, d.numel())       # the test's window holds the whole reach
    assert changed and min(changed) >= lo and max(changed) <= hi, (name, min(changed), max(changed), lo, hi)
    assert min(changed) == lo and max(changed) == hi, (name, "halo not tight", min(changed), max(changed), lo, hi)


def _decoder_stage_fns(sd, resblock, rks, rds, ur, uks, prefix="dec."):
    nk = len(rks)
    fns = [lambda x: O._conv(sd, prefix + "conv_pre", x, padding=3)]
    for i, (u, ku) in enumerate(zip(ur, uks)):
        def stage(x, i=i, u=u, ku=ku):
            x = F.leaky_relu(x, O.LRELU_SLOPE)
            x = F.conv_transpose1d(x, O.conv_weight(sd, f"{prefix}ups.{i}"), O._bias(sd, f"{prefix}ups.{i}"), stride=u, padding=(ku - u) // 2)
            xs = None
            for j, (k, d) in enumerate(zip(rks, rds)):
                rb = O.resblock1 if resblock == "1" else O.resblock2
                y = rb(sd, f"{prefix}resblocks.{i * nk + j}.", x, k, tuple(d))
                xs = y if xs is None else xs + y
            return xs / nk
        fns.append(stage)
    fns.append(lambda x: torch.tanh(F.conv1d(F.leaky_relu(x), sd[prefix + "conv_post.weight"], None, padding=3)))
    return fns


def _check_decoder(geo, sd, cfg, C0, L=40):
    stages = geo["stages"]
    dec = stages[-(len(cfg["ur"]) + 2):]
    fns = _decoder_stage_fns(sd, cfg["resblock"], cfg["rks"], cfg["rds"], cfg["ur"], cfg["uks"])
    g = torch.Generator().manual_seed(5)
    C = C0
    for s, fn in zip(dec, fns):
        rate_in = s["rate"] // s["u"]
        Lin = L * rate_in
        x = torch.randn(1, C, Lin, generator=g, dtype=torch.float64)
        _check_reach(fn, x, Lin // 2, s["u"], s["h_left"], s["h_right"], s["name"])
        with torch.no_grad():
            C = fn(x).shape[1]


def test_geometry_iitp_base_decoder(built):
    geo = _geometry(built, **IITP)
    sd = _f64({k: v for k, v in cases.full_model_weights(skip_enc_q=True).items() if k.startswith("dec.")})
    _check_decoder(geo, sd, IITP, 192)


def test_geometry_iitp_base_encoder_and_couplings(built):
    geo = _geometry(built, **IITP)
    st = geo["stages"]
    assert [s["name"] for s in st[:6]] == ["encoder"] + [f"coupling.{j}" for j in range(4)] + ["conv_pre"]
    sd = _f64({k: v for k, v in cases.full_model_weights(skip_enc_q=True).items() if k.startswith(("enc_p.", "flow."))})
    L = 80
    g = torch.Generator().manual_seed(6)
    mel = torch.randn(1, 80, L, generator=g, dtype=torch.float64)
    eps = torch.randn(1, 192, L, generator=g, dtype=torch.float64)
    ln = torch.tensor([L])

    def enc(x):
        _, m, logs, _ = O.mel_encoder(sd, x, ln)
        return m + eps * torch.exp(logs) * 0.667
    _check_reach(enc, mel, L // 2, 1, st[0]["h_left"], st[0]["h_right"], "encoder")
    mask = torch.ones(1, 1, L, dtype=torch.float64)
    z = torch.randn(1, 192, L, generator=g, dtype=torch.float64)
    for j in range(4):   # run order: flows.6, .4, .2, .0, each behind a Flip (oracle flow(reverse=True))
        i = 3 - j
        fn = (lambda x, i=i: O.coupling(sd, f"flow.flows.{2 * i}.", torch.flip(x, [1]), mask, reverse=True))
        s = st[1 + j]
        assert s["u"] == 1 and s["rate"] == 1
        _check_reach(fn, z, L // 2, 1, s["h_left"], s["h_right"], s["name"])


@pytest.mark.parametrize("name", list(cases.GENERATOR_CASES))
def test_geometry_small_generators(built, name):
    c = cases.GENERATOR_CASES[name]
    cfg = dict(resblock=c["resblock"], rks=c["rks"], rds=c["rds"], ur=c["ur"], uic=c["uic"], uks=c["uks"])
    geo = _geometry(built, initial_channel=c["initial_channel"], **cfg)
    sd = _f64(sw.fill_state_dict(cases.generator_shapes(c, "dec."), seed=c["seed"]))
    _check_decoder(geo, sd, cfg, c["initial_channel"])


@pytest.mark.parametrize("cfg", [IITP, dict(resblock="2", rks=[3, 5], rds=[[1, 3], [1, 3]], ur=[2, 2], uic=64, uks=[4, 4])])
def test_lookahead_is_the_sum_of_the_right_halos(built, cfg):
    from fractions import Fraction
    geo = _geometry(built, **cfg)
    hop = math.prod(cfg["ur"])
    assert geo["hop"] == hop
    rates = [s["rate"] for s in geo["stages"]]
    assert rates[-1] == hop and all(r >= 1 for r in rates)
    total = sum(Fraction(s["h_right"], s["rate"]) for s in geo["stages"])
    assert geo["lookahead_frames"] == math.ceil(total)


def test_lookahead_iitp_base_is_below_the_infer_stream_halo(built):
    from smart_vocoder_amd import models
    geo = _geometry(built, **IITP)
    # 32 (encoder) + 4 x 16 (couplings) + 3 (conv_pre) + 64 / 8 + 64 / 64 + 61 / 128 + 61 / 256 + 3 / 256 -> 109
    assert geo["lookahead_frames"] == 109
    assert geo["lookahead_frames"] < models.SynthesizerTrn.RECEPTIVE_FRAMES


def test_geometry_rejects_bad_config(built):
    from smart_vocoder_amd import models
    c = _synth_config(built, models, **IITP)
    c.dec.upsample_kernel_sizes[0] = 15
    assert built.lib().svoc_stream_geometry(c, None, 0) < 0
    assert b"upsample" in built.lib().svoc_last_error()
