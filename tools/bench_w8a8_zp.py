"""Cost of activation zero points in the fused W8A8 encoder engine, and in its attention kernels alone.

Encoder: ``random_fq_encoder("vit_b", img_size=1024)``, one image, the forward captured in a HIP graph
and replayed (as ``bench.py --mode w8a8`` does), ms per image of
  sym        the symmetric engine (minmax calibration);
  zp0        the zero-point engine on the same calibration (every zero point 0: the same codes);
  zp-omse    the zero-point engine on an omse calibration (non-zero zero points).
The variants are timed interleaved, ``--rounds`` times; the median and the spread are printed.
Attention: ``samq_rel_attention_q8_zp`` against ``samq_rel_attention_q8_rows`` (int8 V and, on the
64 x 64 grid, the fp16 V copy the symmetric engine uses) at window 14 and on the global grid, HIP events
around ``--iters`` launches, best of three.

``--ptf``: the cost of Power-of-Two Factor activations instead -- the zero-point engine on a uint8
calibration with and without ``ptf`` (same weights and images), the ``neck[0]`` replay GEMM alone against
the plain ``samq_i8_gemm_zp`` at M = 4096, N = 256, K = 768, and (reported only) the accuracy of both
engines against the float module graph.

    python tools/bench_w8a8_zp.py [--rounds 5] [--replays 20] [--iters 20] [--skip-encoder] [--ptf]
"""
import argparse
import statistics
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "sam-quantization_amd"))
from samq import ops  # noqa: E402
from samq.synthetic import random_fq_encoder  # noqa: E402


def _time(fn, iters):
    stream = torch.cuda.current_stream()
    best = 1e9
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(iters):
            fn()
        e1.record(stream)
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) / iters)
    return best


def bench_attention(iters):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    heads, d, side = 12, 64, 64
    c = heads * d
    qkv = torch.randint(-100, 100, (1, side, side, 3 * c), generator=g, device=dev, dtype=torch.int8)
    bias = torch.randn(3 * c, generator=g, device=dev) * 0.1
    for window in (14, 0):
        s = 2 * (window or side) - 1
        rh = torch.randn(s, d, generator=g, device=dev) * 0.1
        rw = torch.randn(s, d, generator=g, device=dev) * 0.1
        args = (qkv, bias if window else None, rh, rw, heads, window, d ** -0.5, 0.05, 0.08, 0.1, 0.03)
        sym = _time(lambda: ops.rel_attention_q8(*args), iters)
        zp = _time(lambda: ops.rel_attention_q8_zp(*args, 23, -9, 17, -31), iters)
        line = f"attention vit_b window={window:2d}: symmetric {sym * 1e3:7.1f} us, zero points {zp * 1e3:7.1f} us ({zp / sym:.3f}x)"
        if window == 0:
            v16 = qkv[..., 2 * c:].to(torch.float16).contiguous()
            s16 = _time(lambda: ops.rel_attention_q8(*args, v16=v16), iters)
            line += f"; symmetric with fp16 V {s16 * 1e3:7.1f} us ({zp / s16:.3f}x)"
        print(line, flush=True)


def bench_encoder(rounds, replays):
    dev = torch.device("cuda:0")
    img = torch.randn((1, 3, 1024, 1024), generator=torch.Generator(device=dev).manual_seed(5), device=dev)
    sym_enc = random_fq_encoder("vit_b", device=dev, img_size=1024)
    omse_enc = random_fq_encoder("vit_b", device=dev, img_size=1024, quant_method="omse")
    engines = {"sym": sym_enc.engine(), "zp0": sym_enc.engine(zero_points=True),
               "zp-omse": omse_enc.engine(zero_points=True)}
    graphs = {k: e.capture(img) for k, e in engines.items()}
    assert torch.equal(graphs["sym"][1], graphs["zp0"][1]), "zero zero points must give the symmetric codes"
    times = {k: [] for k in engines}
    stream = torch.cuda.current_stream()
    for _ in range(rounds):
        for k, (graph, _) in graphs.items():
            graph.replay()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(replays):
                graph.replay()
            e1.record(stream)
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) / replays)
    base = statistics.median(times["sym"])
    for k, t in times.items():
        med = statistics.median(t)
        print(f"encoder vit_b 1024 {k:8s}: median {med:.4f} ms per image (min {min(t):.4f}, max {max(t):.4f}), "
              f"{med / base:.3f}x symmetric", flush=True)


def bench_ptf(rounds, replays, iters):
    import copy
    dev = torch.device("cuda:0")
    img = torch.randn((1, 3, 1024, 1024), generator=torch.Generator(device=dev).manual_seed(5), device=dev)
    encs = {"zp-uint8": random_fq_encoder("vit_b", device=dev, img_size=1024, act_bit_type="uint8"),
            "zp-uint8-ptf": random_fq_encoder("vit_b", device=dev, img_size=1024, act_bit_type="uint8", ptf=True,
                                              lis=True)}
    flt = {}
    for k, enc in encs.items():   # the float module graph of the same weights (before an engine exists)
        f = copy.deepcopy(enc)
        f.model_dequant()
        with torch.no_grad():
            flt[k] = f.module_forward(img).float()
        del f
    engines = {k: e.engine(zero_points=True) for k, e in encs.items()}
    graphs = {k: e.capture(img) for k, e in engines.items()}
    times = {k: [] for k in engines}
    stream = torch.cuda.current_stream()
    for _ in range(rounds):
        for k, (graph, _) in graphs.items():
            graph.replay()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(replays):
                graph.replay()
            e1.record(stream)
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) / replays)
    base = statistics.median(times["zp-uint8"])
    for k, t in times.items():
        med = statistics.median(t)
        print(f"encoder vit_b 1024 {k:13s}: median {med:.4f} ms per image (min {min(t):.4f}, max {max(t):.4f}), "
              f"{med / base:.3f}x zp-uint8", flush=True)
    for k, (_, out) in graphs.items():   # accuracy against the float graph, in steps of the output quantiser
        s = float(encs[k].qacts[3].quantizer.scale)
        d = (out.float() - flt[k]).abs() / s
        cos = torch.nn.functional.cosine_similarity(out.float().reshape(1, -1), flt[k].reshape(1, -1)).item()
        print(f"accuracy {k:13s}: mean |dcode| {d.mean().item():.3f} against the float module graph, cosine {cos:.5f}",
              flush=True)
    eng = engines["zp-uint8-ptf"]
    lw, q_in = eng.neck0, eng.blocks[-1]["q"]["x2"]
    x = torch.randint(-128, 128, (4096, 768), device=dev, dtype=torch.int8)
    plain = encs["zp-uint8"].engine(zero_points=True).neck0
    t_rep = _time(lambda: eng._gemm_zp(x, lw, ops.EPI_Q8, q_in, eng.q_neck[0], e_out=eng.e_neck[0]), iters)
    t_zp = _time(lambda: ops.i8_gemm_zp(x, plain["packed"], plain["scale"], 256, None, ops.EPI_Q8, q_in[0],
                                        eng.q_neck[0][0], col_offset=plain["col_offset"]), iters)
    print(f"neck[0] M=4096 N=256 K=768: samq_i8_gemm_zp {t_zp * 1e3:.1f} us, replay ({lw['passes']} passes) "
          f"{t_rep * 1e3:.1f} us ({t_rep / t_zp:.2f}x)", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--skip-encoder", action="store_true")
    ap.add_argument("--ptf", action="store_true")
    args = ap.parse_args()
    if args.ptf:
        return bench_ptf(args.rounds, args.replays, args.iters)
    bench_attention(args.iters)
    if not args.skip_encoder:
        bench_encoder(args.rounds, args.replays)


if __name__ == "__main__":
    main()
