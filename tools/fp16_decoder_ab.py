"""A/B of the decoder's fp16 mode (decoder_precision="fp16") against the fp32 default, in one process on one GPU.

For 16 x 512, 4 x 512 and 1 x 200 frames (bench.py's synthetic mel / eps, seed 1001): warm-up, then the median of 20
SynthesizerTrn.infer calls per mode, each timed with HIP events on the current stream, and the relative RMS difference of the
two waveforms.  Then one profiled fp16 call at 16 x 512 (svoc_profile_report: per-shape launch times).
Usage: python tools/fp16_decoder_ab.py [--iters 20] [--warmup 5] [--out profiles/fp16_decoder_ab.txt]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import cases
    from cases import sw
    from smart_vocoder_amd import models, _native as N
    torch.cuda.set_device(0)
    net = models.SynthesizerTrn(513, 32, n_speakers=109, **cases.IITP_MODEL)
    sd = cases.full_model_weights(skip_enc_q=True)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    net = net.cuda().eval()
    lines = [f"device: {torch.cuda.get_device_name(0)}; median of {a.iters} infer calls after {a.warmup} warm-up calls, HIP events"]

    def timed(mel, ln, eps, prec):
        for _ in range(a.warmup):
            net.infer(mel, ln, noise_scale=0.667, eps=eps, decoder_precision=prec)
        ts = []
        for _ in range(a.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            o = net.infer(mel, ln, noise_scale=0.667, eps=eps, decoder_precision=prec)[0]
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        return statistics.median(ts), o.cpu().numpy().astype(np.float64)

    with torch.no_grad():
        for B, T in ((16, 512), (4, 512), (1, 200)):
            mel = torch.from_numpy(sw.synthetic_mel(1001, B, T)).cuda()
            eps = torch.from_numpy(sw.synthetic_eps(1001, B, T)).cuda()
            ln = torch.full((B,), T, dtype=torch.int64).cuda()
            net.reserve(B, T)
            t32, o32 = timed(mel, ln, eps, "fp32")
            t16, o16 = timed(mel, ln, eps, "fp16")
            rel = float(np.sqrt(((o16 - o32) ** 2).mean()) / np.sqrt((o32 ** 2).mean()))
            lines.append(f"{B:2d} x {T}: fp32 {t32:8.3f} ms   fp16 {t16:8.3f} ms   fp16/fp32 {t16 / t32:.3f}   waveform rel-RMS fp16 vs fp32 {rel:.2e}")
            print(lines[-1], flush=True)
        B, T = 16, 512
        mel = torch.from_numpy(sw.synthetic_mel(1001, B, T)).cuda()
        eps = torch.from_numpy(sw.synthetic_eps(1001, B, T)).cuda()
        ln = torch.full((B,), T, dtype=torch.int64).cuda()
        N.profile_enable(True)
        net.infer(mel, ln, noise_scale=0.667, eps=eps, decoder_precision="fp16")
        torch.cuda.synchronize()
        rep = N.profile_report()
        N.profile_enable(False)
        lines.append("svoc_profile_report, one fp16 infer at 16 x 512:")
        lines.append(rep.rstrip())
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
