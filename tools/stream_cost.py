"""Per-frame cost of streaming: InferStream (net.stream()) against StatefulStream (net.stream(carry_state=True)), with one-shot infer at
16 x 512 as the baseline.  Device events around every push; the median of the pushes after warm-up, divided by the frames the push
carries (B x push).  The two streams alternate push by push on one net, so clocks and power state are shared.

    python tools/stream_cost.py [--pushes 24] [--warmup 4]    (profiles/stream_state_cost.txt is its output)"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

import cases  # noqa: E402
from cases import sw  # noqa: E402


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pushes", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=4)
    args = ap.parse_args()
    from smart_vocoder_amd import models
    net = models.SynthesizerTrn(513, 32, n_speakers=109, **cases.IITP_MODEL)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in cases.full_model_weights(skip_enc_q=True).items()}, strict=False)
    net = net.cuda().eval()
    print(f"device: {torch.cuda.get_device_name(0)}; lookahead: StatefulStream {net.stream(carry_state=True).lookahead_frames} frames, "
          f"InferStream {net.RECEPTIVE_FRAMES} frames")

    # baseline: one-shot infer 16 x 512
    B, T = 16, 512
    mel = torch.from_numpy(sw.synthetic_mel(1001, B, T)).cuda()
    eps = torch.from_numpy(sw.synthetic_eps(1001, B, T)).cuda()
    ln = torch.full((B,), T, dtype=torch.int64, device="cuda")
    with torch.no_grad():
        for _ in range(3):
            net.infer(mel, ln, noise_scale=0.667, eps=eps)
        ts = [_timed(lambda: net.infer(mel, ln, noise_scale=0.667, eps=eps))[0] for _ in range(10)]
    base = statistics.median(ts) / (B * T)
    print(f"one-shot infer 16 x 512: {statistics.median(ts):.2f} ms, {base * 1e3:.2f} us per frame")
    print()
    print(f"{'B':>3} {'push':>5} {'InferStream us/frame':>21} {'Stateful us/frame':>18} {'stateful/infer_stream':>22} "
          f"{'stateful/one-shot':>18}")
    for B in (16, 1):
        for P in (40, 160):
            n = args.warmup + args.pushes
            T = n * P
            mel = torch.from_numpy(sw.synthetic_mel(2000 + P, B, T)).cuda()
            eps = torch.from_numpy(sw.synthetic_eps(2000 + P, B, T)).cuda()
            old = net.stream(noise_scale=0.667)
            new = net.stream(noise_scale=0.667, carry_state=True, max_chunk_frames=P)
            t_old, t_new = [], []
            with torch.no_grad():
                for i in range(n):
                    m, e = mel[:, :, i * P:(i + 1) * P].contiguous(), eps[:, :, i * P:(i + 1) * P].contiguous()
                    a, _ = _timed(lambda: old.push(m, e))
                    b, _ = _timed(lambda: new.push(m, e))
                    if i >= args.warmup:
                        t_old.append(a)
                        t_new.append(b)
                old.flush()
                new.flush()
            fo, fn = statistics.median(t_old) / (B * P), statistics.median(t_new) / (B * P)
            print(f"{B:>3} {P:>5} {fo * 1e3:>21.2f} {fn * 1e3:>18.2f} {fn / fo:>22.2f} {fn / base:>18.2f}")
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
