"""CPU checks of the decoder's opt-in fp16 mode (decoder_precision=): bad values are refused before any device work, and the
binding carries the new C entry points (include/svoc.h, ABI 7)."""
import pytest
import torch

import cases

BAD = ["bf16", 1, "half", None, "FP16"]


def _net():
    from smart_vocoder_amd import models
    return models.SynthesizerTrn(513, 32, n_speakers=109, **cases.IITP_MODEL)


@pytest.mark.parametrize("bad", BAD)
def test_infer_family_rejects_unknown_precision(bad):
    net = _net()
    mel = torch.zeros(1, 80, 8)
    ln = torch.tensor([8])
    with pytest.raises(ValueError, match="decoder_precision"):
        net.infer(mel, ln, noise_scale=0.0, decoder_precision=bad)
    with pytest.raises(ValueError, match="decoder_precision"):
        net.infer_chunked(mel, ln, chunk_frames=4, noise_scale=0.0, decoder_precision=bad)
    with pytest.raises(ValueError, match="decoder_precision"):
        net.stream(noise_scale=0.0, decoder_precision=bad)


@pytest.mark.parametrize("bad", BAD)
def test_generator_forward_rejects_unknown_precision(bad):
    from smart_vocoder_amd import models
    g = models.Generator(32, "1", [3], [[1, 3, 5]], [2], 32, [4])
    with pytest.raises(ValueError, match="decoder_precision"):
        g(torch.zeros(1, 32, 8), decoder_precision=bad)


def test_precision_is_keyword_only():
    import inspect
    from smart_vocoder_amd import models
    for fn in (models.SynthesizerTrn.infer, models.SynthesizerTrn.infer_chunked, models.SynthesizerTrn.stream,
               models.Generator.forward, models.InferStream.__init__):
        p = inspect.signature(fn).parameters["decoder_precision"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == "fp32", fn


def test_binding_carries_fp16_entry_points():
    from smart_vocoder_amd import _native as N
    assert N.ABI_VERSION == 7
    for name in ("svoc_synth_set_decoder_precision", "svoc_generator_set_decoder_precision", "svoc_conv1d_f16"):
        assert name in N.SIGNATURES, name
    assert N.SIGNATURES["svoc_conv1d_f16"][1] == N.SIGNATURES["svoc_conv1d"][1]


class _RecordingNet:
    """CPU stand-in for SynthesizerTrn that records the decoder_precision each infer call receives."""
    RECEPTIVE_FRAMES = 5
    inter_channels = 3

    class dec:
        hop = 4

    def __init__(self):
        self.seen = []

    def infer(self, mel, ln, noise_scale=1, eps=None, max_len=None, **kw):
        self.seen.append(kw.get("decoder_precision", "fp32"))
        return (mel[:, :1] + noise_scale * eps[:, :1]).repeat_interleave(4, dim=2), None, None

    def _dev(self):
        return torch.device("cpu")


@pytest.mark.parametrize("prec", ["fp16", "fp32"])
def test_chunked_and_stream_pass_precision_on(monkeypatch, prec):
    from smart_vocoder_amd import models, _native
    monkeypatch.setattr(_native, "f32", lambda t: t.float().contiguous())
    g = torch.Generator().manual_seed(5)
    mel = torch.randn(2, 80, 40, generator=g); eps = torch.randn(2, 3, 40, generator=g)
    net = _RecordingNet()
    models.SynthesizerTrn.infer_chunked(net, mel, torch.tensor([40, 40]), chunk_frames=16, noise_scale=0.5, eps=eps, decoder_precision=prec)
    assert len(net.seen) == 3 and set(net.seen) == {prec}
    net.seen.clear()
    s = models.InferStream(net, noise_scale=0.5, decoder_precision=prec)
    for a in range(0, 40, 9):
        s.push(mel[:, :, a:a + 9], eps[:, :, a:a + 9])
    s.flush()
    assert len(net.seen) >= 2 and set(net.seen) == {prec}
