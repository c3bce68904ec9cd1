#!/usr/bin/env python3
"""Benchmark: 1024x1024 images/sec through the quantized SAM image encoder.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--batch B] [--mode w4a16|w4a8|w8a8]
                    [--full] [--dump-outputs DIR]

Default (the headline, BASELINE config 3/4): ``--mode w4a16`` = ViT-H GPTQ int4 weights x fp16
activations.  ``--mode w4a8`` (config 5): ViT-H int4 weights x int8 activations on the int8 MFMA,
batch 8.  ``--mode w8a8`` (config 2): vit_b fq_vit W8A8, batch 1.

One process per GPU.  Under ``torch.distributed.run`` (RANK / LOCAL_RANK / WORLD_SIZE /
MASTER_* in the env) every process is one rank.  Started bare with ``--gpus N > 1`` the script
launches its own N ranks: it starts ``torch.distributed.run`` as a CHILD process before anything
touches the GPU, relays rank 0's line and exits with the child's status (the reference's
``mp.spawn`` + ``init_process_group`` pattern, train_sm.py:587-590, 630-636, without re-exec).
A "step" = one encoder forward over the per-GPU batch of synthetic images already resident in
HBM (a HIP-graph replay of the fused engine).  Weights are random-init ViT-H, RTN-quantised into
the reference's packed int4 format on rank 0 and RCCL-broadcast to the other ranks (the only
collective on the data path).  One seeded global batch (image i drawn from seed 1234 + i) is
sharded contiguously over the ranks (``samq.dist.shard``); per-GPU work is fixed ("weak"
scaling): 4 images per GPU at N=1 (BASELINE config 3), 8 per GPU at N>1 (config 4 at N=8 =
global batch 64).

A plain run sets up, warms up, times the steps and prints the throughput line; its roofline stanza
quotes the committed in-step profile of this build when there is one.  ``--dump-outputs DIR``
also writes rank 0's encoder output of the last timed step to ``DIR/image_embeddings.npy``
(weights and images are seeded: the same arguments give the same inputs in every run).

``--full`` adds, after the timed steps: the isolated-launch roofline figure of the dominant kernel
(all projection GEMM launches of one forward) next to the in-step one, the CPU baseline (the
oracle restatement of the reference's fp32 CPU fake-quant path, median of 3 one-image runs after
one warm-up, rank 0, N=1), parity + mask IoU of the timed graph's own output against the oracle,
and, in a 1-GPU W4A16 run, the W4A8 (config 5) and W8A8 (config 2) sub-records.

``--dry-run --backend gloo`` exercises the launcher / sharding / weight broadcast on the CPU
(tiny model, no GPU) for the multi-process tests.
"""
from __future__ import annotations

import argparse
import json
import os
import socket
import statistics
import subprocess
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent
sys.path.insert(0, str(REPO / "sam-quantization_amd"))

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

METRIC = "1024×1024 images/sec through quantized ViT-H encoder; % of MFMA/HBM roofline"
PEAK_FP16_TFLOPS = 2500.0   # MI355X dense fp16/bf16 MFMA (MI355X_MICROARCH.md)
PEAK_HBM_GBS = 8000.0


def log(*a):
    print(*a, file=sys.stderr, flush=True)


# committed PMC passes (tools/pmc_all.sh) per (mode, GEMM rows per launch), newest round first
PMC_PROFILES = {("w4a16", 16384): ["r1_pmc_traffic_w4a16.json"],
                ("w4a16", 8192): ["r6_pmc_traffic_w4a16_m8192.json", "r5_pmc_traffic_w4a16_m8192.json"],
                ("w4a8", 16384): ["r6_pmc_traffic_w4a8_m16384.json", "r5_pmc_traffic_w4a8_m16384.json"],
                ("w8a8", 4096): ["r6_pmc_traffic_w8a8_m4096.json", "r5_pmc_traffic_w8a8_m4096.json"]}


def pmc_traffic(mode: str, profiles):
    """HBM bytes per launch of the mode's projection GEMMs (``is_proj_gemm``; dispatch-weighted
    average) from the newest committed rocprofv3 PMC summary (tools/pmc_all.sh -> profiles/*.json),
    or None."""
    found = [p for p in ([profiles] if isinstance(profiles, str) else profiles) if (REPO / "profiles" / p).exists()]
    if not found:
        return None, None
    profile = found[0]
    f = REPO / "profiles" / profile
    d = json.loads(f.read_text())
    tot = n = 0
    for k, v in d["kernels"].items():
        if is_proj_gemm(mode, k) and v.get("hbm_bytes_avg"):
            tot += v["hbm_bytes_avg"] * v["dispatches"]
            n += v["dispatches"]
    return (round(tot / n) if n else None), f"profiles/{profile}: " + d["source"]


def gemm_roofline(eng, bufs_batch: int, reps: int = 3):
    """ISOLATED figure: average duration of every W4A16 GEMM launch of one forward at
    ``bufs_batch`` images per launch (one lane), HIP events on the launch stream, launches back to
    back with no concurrent lane; achieved = algorithmic FLOPs (2*M*N*K per launch) / duration.
    The headline ``roofline`` comes from ``step_profile`` (inside the timed graph)."""
    from samq import ops
    bufs = eng.buffers(bufs_batch)
    stream = torch.cuda.current_stream()
    rows = bufs["x"].numel() // bufs["x"].shape[-1]
    records = []
    for _ in range(reps):
        for p in eng.plans:
            for lin, a, out, epi in ((p.qkv, bufs["xn"], bufs["qkv"], ops.EPI_BIAS),
                                     (p.proj, bufs["att"], bufs["x"], ops.EPI_RESADD_F32),
                                     (p.lin1, bufs["xn"], bufs["hid"], ops.EPI_BIAS_GELU),
                                     (p.lin2, bufs["hid"], bufs["x"], ops.EPI_RESADD_F32)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                lin.forward_epilogue(a, epi, out=out)
                e1.record(stream)
                records.append((e0, e1, 2.0 * rows * lin.infeatures * lin.outfeatures))
    torch.cuda.synchronize()
    t = sum(e0.elapsed_time(e1) for e0, e1, _ in records) / 1e3
    flops = sum(f for *_, f in records)
    n = len(records)
    achieved = flops / t / 1e12
    # algorithmic bytes per launch (A f16 in, packed int4 W, output f16 or f32 read-modify-write)
    alg = []
    for p in eng.plans:
        for lin, out_b in ((p.qkv, 2), (p.proj, 8), (p.lin1, 2), (p.lin2, 8)):
            alg.append(rows * lin.infeatures * 2 + lin.infeatures * lin.outfeatures // 2 + rows * lin.outfeatures * out_b)
    # committed PMC passes per GEMM row count: M = 16384 (one B=4 chain), M = 8192 (a 2-image lane)
    prof = PMC_PROFILES.get(("w4a16", rows))
    traffic, src = pmc_traffic("w4a16", prof) if prof else (None, None)
    return dict(bound="mfma", achieved=round(achieved, 1), peak=PEAK_FP16_TFLOPS, unit="TFLOP/s",
                frac=round(achieved / PEAK_FP16_TFLOPS, 4), traffic=traffic,
                traffic_unit="bytes per launch (L2->fabric, PMC)", traffic_source=src,
                algorithmic_bytes_per_launch=round(sum(alg) / len(alg)),
                kernel="w4a16_gemm_pp2 (qkv, lin1) + w4a16_gemm_v3 (proj, lin2): all 4 ViT-H projection shapes",
                launches_timed=n,
                avg_launch_us=round(t / n * 1e6, 2))


PEAK_INT8_TOPS = 5000.0     # MI355X dense int8 MFMA (2x fp16, MI355X_MICROARCH.md)

# committed rocprofv3 --kernel-trace --stats summaries of the timed configuration itself, one per
# kernel-source build: `tools/instep_profile.sh` runs `rocprofv3 --kernel-trace --stats -- python3
# bench.py --steps 10 --warmup 3 --no-cpu-baseline --no-isolated` (every GEMM dispatch in it is a
# graph replay or capture warm-up with the timed lanes) and commits the kernel stats as
# profiles/instep_<mode>_b<images per launch>_l<lanes>_<source hash>.csv


def source_hash() -> str:
    """sha1 of the HIP sources + build recipe the library is compiled from (12 hex digits)."""
    import hashlib
    h = hashlib.sha1()
    pkg = REPO / "sam-quantization_amd"
    for f in sorted(list((pkg / "csrc").glob("*")) + [pkg / "Makefile", REPO / "include" / "samq.h"]):
        h.update(f.name.encode())
        h.update(f.read_bytes())
    return h.hexdigest()[:12]


def _roctx():
    try:
        import ctypes
        return ctypes.CDLL("librocprofiler-sdk-roctx.so.1")
    except OSError:
        return None


def is_proj_gemm(mode, name):
    """Is a dispatch one of the mode's projection GEMMs (qkv / proj / lin1 / lin2 [+ the W8A8 neck
    1x1, an int8 GEMM of the same kernel)?  i8_gemm_kernel<BM, BN, WM, WN, EPI, W4, ., AG>: W4
    selects the int4-weight form, AG = 0 the plain row-major A operand (not the implicit convs)."""
    if mode == "w4a16":
        return "w4a16_gemm" in name
    if mode == "w4a8" and "i8_gemm_pp2<" in name:   # the int4-weight ping-pong GEMM (M >= 8192)
        return True
    if "i8_gemm_kernel<" not in name:
        return False
    args = [a.strip() for a in name.split("i8_gemm_kernel<", 1)[1].split(">", 1)[0].split(",")]
    return args[5] == ("1" if mode == "w4a8" else "0") and args[7] == "0"


def instep_name(mode, imgs_per_launch, lanes, groupsize=-1):
    g = f"_g{groupsize}" if groupsize and groupsize > 0 else ""
    return f"instep_{mode}{g}_b{imgs_per_launch}_l{lanes}_{source_hash()}"


def in_step_from_profile(mode, imgs_per_launch, lanes, flops_step, peak, groupsize=-1):
    """GEMM roofline of the timed replays (concurrent lanes included) from the committed rocprof
    kernel trace, restricted to bench's roctx-marked timed window: GEMM FLOPs of the window /
    summed GEMM dispatch time (tools/instep_profile.sh writes the JSON)."""
    name = instep_name(mode, imgs_per_launch, lanes, groupsize) + ".json"
    f = REPO / "profiles" / name
    if not f.exists() or not flops_step:
        return None
    d = json.loads(f.read_text())
    tot_ns = n = 0
    for k, v in d["kernels"].items():
        if is_proj_gemm(mode, k):
            tot_ns += v["total_ns"]
            n += v["calls"]
    if not n:
        return None
    flops = flops_step * d["steps"]
    summed = flops / (tot_ns * 1e-9) / 1e12
    # headline: GEMM FLOPs over the time during which at least one GEMM ran (the union of their
    # dispatch intervals); the summed per-dispatch durations count the lanes' overlap twice
    uni = d.get("gemm_union_ns")
    ach = flops / (uni * 1e-9) / 1e12 if uni else summed
    return dict(achieved=round(ach, 1), frac=round(ach / peak, 4), avg_launch_us=round(tot_ns / n / 1e3, 2),
                method=("GEMM FLOPs of the timed window / union of the GEMM dispatch intervals" if uni else
                        "GEMM FLOPs of the timed window / summed GEMM dispatch durations"),
                summed_durations=dict(achieved=round(summed, 1), frac=round(summed / peak, 4)),
                gemm_busy_frac_of_window=round(uni / (d["window_ms"] * 1e6), 4) if uni else None,
                dispatches=n, steps=d["steps"], window_ms=d["window_ms"], source=f"profiles/{name}")


def _time_launches(launches, reps=3):
    """launches: list of (callable, flops); returns (total seconds, total flops, count)."""
    stream = torch.cuda.current_stream()
    records = []
    for _ in range(reps):
        for fn, fl in launches:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            records.append((e0, e1, fl))
    torch.cuda.synchronize()
    t = sum(e0.elapsed_time(e1) for e0, e1, _ in records) / 1e3
    return t, sum(f for *_, f in records), len(records)


def w4a8_roofline(eng, batch: int):
    from samq import ops
    bufs = eng.buffers(batch)
    rows = bufs["x"].numel() // bufs["x"].shape[-1]
    launches = []
    for p in eng.plans:
        for lin, a, s, out, epi, so in ((p.qkv, "xn8", p.s_qkv, "qkv", ops.EPI_BIAS, 0.0),
                                        (p.proj, "att8", p.s_proj, "x", ops.EPI_RESADD_F32, 0.0),
                                        (p.lin1, "xn8", p.s_lin1, "hid8", ops.EPI_Q8_GELU, p.s_lin2),
                                        (p.lin2, "hid8", p.s_lin2, "x", ops.EPI_RESADD_F32, 0.0)):
            launches.append((lambda lin=lin, a=a, s=s, out=out, epi=epi, so=so:
                             lin.forward_w4a8(bufs[a], s, epi, out=bufs[out], out_scale=so),
                             2.0 * rows * lin.infeatures * lin.outfeatures))
    t, fl, n = _time_launches(launches)
    achieved = fl / t / 1e12
    return dict(bound="mfma", achieved=round(achieved, 1), peak=PEAK_INT8_TOPS, unit="TFLOP/s",
                frac=round(achieved / PEAK_INT8_TOPS, 4), traffic=None,
                kernel="i8_gemm_pp2 / i8_gemm_kernel W4 (int4 x int8 MFMA, all 4 ViT-H projection shapes)", launches_timed=n,
                avg_launch_us=round(t / n * 1e6, 2))


def w8a8_roofline(eng, batch: int):
    from samq import ops
    dev = eng.dev
    c = eng.embed_dim
    rows = batch * (eng.enc.img_size // eng.patch) ** 2
    a = torch.randint(-100, 100, (rows, 4 * c), dtype=torch.int8, device=dev)
    x = torch.randint(-100, 100, (rows, c), dtype=torch.int8, device=dev)
    launches = []
    for bl in eng.blocks:
        for lw, epi, k in ((bl["qkv"], ops.EPI_Q8, c), (bl["proj"], ops.EPI_Q8_RES, c),
                           (bl["lin1"], ops.EPI_Q8_GELU, c), (bl["lin2"], ops.EPI_Q8_RES, 4 * c)):
            res = x if epi == ops.EPI_Q8_RES else None
            launches.append((lambda lw=lw, epi=epi, k=k, res=res: eng._gemm(a[:, :k], lw, epi, 0.01, 0.05, mid=0.05,
                                                                         res=res, res_scale=0.05),
                             2.0 * rows * lw["k"] * lw["n"]))
    t, fl, n = _time_launches(launches)
    achieved = fl / t / 1e12
    return dict(bound="mfma", achieved=round(achieved, 1), peak=PEAK_INT8_TOPS, unit="TFLOP/s",
                frac=round(achieved / PEAK_INT8_TOPS, 4), traffic=None,
                kernel="i8_gemm_kernel W8 (int8 x int8 MFMA, vit_b projection shapes)", launches_timed=n,
                avg_launch_us=round(t / n * 1e6, 2))


def gemm_shapes(mode, eng):
    """Per block: the (K, N) of qkv, proj, lin1, lin2."""
    if mode == "w8a8":
        return [tuple((bl[k]["k"], bl[k]["n"]) for k in ("qkv", "proj", "lin1", "lin2")) for bl in eng.blocks]
    return [tuple((lin.infeatures, lin.outfeatures) for lin in (p.qkv, p.proj, p.lin1, p.lin2)) for p in eng.plans]


def gemm_flops_per_step(mode, eng, images):
    """Algorithmic FLOPs of the projection GEMMs (is_proj_gemm) of one step over ``images``."""
    tok = images * 4096
    if mode == "w8a8":
        c = eng.embed_dim
        tok = images * (eng.enc.img_size // eng.patch) ** 2
        fl = sum(2.0 * tok * bl[k]["k"] * bl[k]["n"] for bl in eng.blocks for k in ("qkv", "proj", "lin1", "lin2"))
        return fl + 2.0 * tok * c * 256                    # neck 1x1 (same kernel form)
    return sum(2.0 * tok * lin.infeatures * lin.outfeatures
               for p in eng.plans for lin in (p.qkv, p.proj, p.lin1, p.lin2))


def oracle_state(enc, cfg, groupsize: int):
    """The bench encoder's own weights in the oracle's (reference) naming: non-Linear parameters
    as fp32 tensors of their fp16 values, every block Linear dequantised from its packed GPTQ
    buffers in G1 semantics (s * (q - zp), oracle/gptq_pack.dequant_g1) -- the checkpoint the
    reference would load (gptq4sam_infer.py:135-141 load_quant)."""
    import numpy as np
    from oracle import sam_ref, synth
    sd = {}
    for k, v in enc.state_dict().items():
        sd[k.replace("attn.qkv_proj.", "attn.qkv.").replace("attn.o_proj.", "attn.proj.")] = v.detach().cpu()
    names = synth.linear_names(cfg)
    q = {}
    for n in names:
        q[n + ".qweight"] = sd[n + ".qweight"].numpy()
        q[n + ".qzeros"] = sd[n + ".qzeros"].numpy()
        q[n + ".scales"] = sd[n + ".scales"].numpy()
    lw = sam_ref.quantized_linear_weights(q, names, groupsize)
    lb = {n: sd[n + ".bias"].float().numpy() for n in names}
    lin = tuple(n + "." for n in names)
    st = {k: v.half().float().numpy() for k, v in sd.items() if not k.startswith(lin) and v.is_floating_point()}
    return st, lw, lb, np


def _cpu_threads(parity_only: bool = False) -> int:
    """Host threads for the oracle: the box's grant (affinity, capped by OMP_NUM_THREADS).  The
    parity-only leg of an N > 1 run (the other ranks idle at a barrier meanwhile) ignores an
    OMP_NUM_THREADS of 1 set by a launcher, up to 16 threads."""
    aff = len(os.sched_getaffinity(0))
    omp = int(os.environ.get("OMP_NUM_THREADS", aff))
    return max(min(aff, omp), min(aff, 16)) if parity_only else min(aff, omp)


def build_oracle(model_name: str, mode: str, enc=None, groupsize: int = -1, precision: str = "fp32"):
    """The mode's oracle (checker side): with the bench encoder ``enc`` it is built from the
    encoder's OWN weights -- W4A16 / W4A8: its packed int4 buffers dequantised (G1) plus, for
    W4A8, its calibrated activation scales; W8A8: its fp32 weights and calibrated QAct scales --
    else from seeded random weights.  ``precision`` "fp64" evaluates the same fake-quant graph in
    float64 (the int8 modes' self-distance reference point).  Returns (oracle, description)."""
    sys.path.insert(0, str(REPO))
    from oracle import sam_ref, synth
    cfg = synth.encoder_config(model_name)
    g = torch.Generator().manual_seed(0)
    own = enc is not None
    dt = {"fp32": torch.float32, "fp64": torch.float64}[precision]
    if mode == "w8a8":
        from oracle import fq_ref
        from samq import fq_vit
        if own:
            st = {k: v.detach().float().cpu().numpy() for k, v in enc.state_dict().items()
                  if v.is_floating_point() and "quantizer" not in k and "observer" not in k}
            scales = {n: float(m.quantizer.scale.reshape(-1)[0]) for n, m in fq_vit.act_quantizers(enc).items()}
        else:
            st = {k: torch.randn(shape, generator=g) * 0.02 for k, shape in _state_shapes(cfg).items()}
            scales = None
        o = fq_ref.FQEncoderOracle(cfg, st, dtype=dt)
        if scales is None:
            qa = ["qact_input", "patch_embed.qact", "qact_pos", "qact1"] + [f"qacts.{i}" for i in range(4)]
            for i in range(cfg["depth"]):
                qa += [f"blocks.{i}.{n}" for n in ("qact1", "qact2", "qact3", "qact4", "attn.qact1", "attn.qact2",
                                                     "attn.qact3", "attn.qact_attn1", "attn.use_rel_pos_qact",
                                                     "mlp.qact1", "mlp.qact2")]
            scales = {n: 0.05 for n in qa}
        o.set_scales(scales)
        return o, "fq_vit W8A8 fake-quant op graph (oracle/fq_ref.py)"
    lw = lb = None
    if own:
        st, lw, lb, _ = oracle_state(enc, cfg, groupsize)
    else:
        st = {k: torch.randn(shape, generator=g) * 0.02 for k, shape in _state_shapes(cfg).items()}
    if mode == "w4a8":
        from oracle import w4a8_ref
        o = w4a8_ref.W4A8EncoderOracle(cfg, st, precision=precision, linear_weights=lw, linear_bias=lb)
        if own:
            from samq import QuantLinear
            o.set_scales({n.replace("qkv_proj", "qkv").replace("o_proj", "proj"): float(m.act_quant.quantizer.scale)
                          for n, m in enc.named_modules() if isinstance(m, QuantLinear)})
        else:
            o.set_scales({n: 0.05 for n in synth.linear_names(cfg)})
        return o, "W4A8 fake-quant op graph (oracle/w4a8_ref.py)"
    return (sam_ref.EncoderOracle(cfg, st, precision=precision, linear_weights=lw, linear_bias=lb),
            "fp32 CPU fake-quant op graph (oracle/sam_ref.py)")


def _oracle_image(img0):
    if img0 is not None:
        return img0.detach().float().cpu().reshape(1, 3, 1024, 1024)
    return torch.randn(1, 3, 1024, 1024, generator=torch.Generator().manual_seed(0))


def cpu_baseline(model_name: str, mode: str = "w4a16", enc=None, img0=None, groupsize: int = -1, runs: int = 3):
    """Oracle restatement of the reference CPU fake-quant path on one 1024x1024 image, rank 0 only,
    median of ``runs`` timed runs after one warm-up (every mode the same method).  With the bench
    encoder (``enc``) and its image 0 (``img0``) the oracle is the encoder's own (``build_oracle``),
    so its output doubles as the parity reference (returned second)."""
    threads = _cpu_threads()
    torch.set_num_threads(threads)
    own = enc is not None and img0 is not None
    o, what = build_oracle(model_name, mode, enc if own else None, groupsize)
    img = _oracle_image(img0 if own else None)
    o(img)   # warm-up (allocator, thread pool)
    times = []
    for _ in range(runs):
        t0 = time.perf_counter()
        ref = o(img)
        times.append(time.perf_counter() - t0)
    dt = statistics.median(times)
    src = "the bench encoder's own weights and image 0" if own else "seeded random weights"
    return dict(value=round(1.0 / dt, 4), unit="img/s", cores=threads, kind="port",
                sample=f"1 image, {model_name} {what} on {src}; median of {runs} runs after 1 warm-up "
                       f"({', '.join(f'{r:.2f}' for r in times)} s), torch {threads} threads, CPU: {_cpu_model()}"
                ), (ref if own else None)


def parity_reference(model_name: str, mode: str, enc, img0, groupsize: int = -1):
    """Parity-only oracle output (N > 1 runs: rank 0's image 0 is global image 0 at every N; no CPU
    baseline is reported there)."""
    torch.set_num_threads(_cpu_threads(parity_only=True))
    o, _ = build_oracle(model_name, mode, enc, groupsize)
    return o(_oracle_image(img0))


def int8_reference_points(model_name: str, mode: str, enc, img0, groupsize: int = -1) -> dict:
    """Reference points for the int8 modes' end-to-end parity (checker side): the SAME fake-quant
    graph evaluated in float64 (``fp64``: how far the oracle's own rounding moves the chaotic int8
    codes) and, for W4A8, the graph without its activation quantisers
    (``int8_noise``: the W4A16 G1 output, tests/test_w4a8.py's noise reference)."""
    torch.set_num_threads(_cpu_threads(parity_only=True))
    img = _oracle_image(img0)
    pts = {}
    o64, _ = build_oracle(model_name, mode, enc, groupsize, precision="fp64")
    pts["fp64"] = o64(img).float()
    del o64
    if mode == "w4a8":
        o, _ = build_oracle(model_name, mode, enc, groupsize)
        o.mode = "float"
        pts["int8_noise"] = o(img)
    return pts


def mask_iou_report(emb: torch.Tensor, ref: torch.Tensor) -> dict:
    """North-star mask IoU, next to the encoder max-abs: the reference's prompt encoder + mask
    decoder (samq/sam_decoder.py, seeded weights = tests/test_sam_decoder.py's) run on the
    engine's embedding of image 0 and on the oracle's, for each fixed prompt of oracle/synth.py
    (points, negative points, a box) with single- and multi-mask output; masks thresholded at 0
    after ``postprocess_masks`` to 1024x1024 (``Sam.forward``); IoU = ``get_iou``
    (script/evaluation2.py:156-167).  Checker side: runs after the timed region."""
    from oracle import synth
    from samq.sam_decoder import build_prompt_decoder, mask_iou, postprocess_masks
    dev = emb.device
    pe, md = build_prompt_decoder()
    shapes = {f"prompt_encoder.{k}": v.shape for k, v in pe.state_dict().items()}
    shapes.update({f"mask_decoder.{k}": v.shape for k, v in md.state_dict().items()})
    st = synth.make_decoder_state(shapes)
    pe.load_state_dict({k[15:]: torch.from_numpy(v) for k, v in st.items() if k.startswith("prompt_encoder.")})
    md.load_state_dict({k[13:]: torch.from_numpy(v) for k, v in st.items() if k.startswith("mask_decoder.")})
    pe, md = pe.to(dev).eval(), md.to(dev).eval()
    ref = ref.to(dev, torch.float32).reshape(emb.shape)
    ious = []
    for pr in synth.DECODER_PROMPTS:
        pts = box = None
        if "points" in pr:
            pts = (torch.tensor([pr["points"]], dtype=torch.float32, device=dev),
                   torch.tensor([pr["labels"]], dtype=torch.int64, device=dev))
        if "box" in pr:
            box = torch.tensor([pr["box"]], dtype=torch.float32, device=dev)
        for mm in (False, True):
            with torch.no_grad():
                sparse, dense = pe(points=pts, boxes=box, masks=None)
                lo_a, _ = md(emb, pe.get_dense_pe(), sparse, dense, mm)
                lo_b, _ = md(ref, pe.get_dense_pe(), sparse, dense, mm)
            for j in range(lo_a.shape[1]):
                a = postprocess_masks(lo_a[:, j:j + 1].float(), 1024, (1024, 1024), (1024, 1024)) > 0.0
                b = postprocess_masks(lo_b[:, j:j + 1].float(), 1024, (1024, 1024), (1024, 1024)) > 0.0
                ious.append(mask_iou(a, b))
    return dict(mask_iou_min=round(min(ious), 5), mask_iou_mean=round(sum(ious) / len(ious), 5), masks=len(ious),
                mask_iou_method="reference prompt encoder + mask decoder (seeded, tests/test_sam_decoder.py) on the "
                                "engine's vs the oracle's image-0 embedding, 5 prompts x single/multi-mask, masks "
                                "at 1024x1024 thresholded at 0; IoU = get_iou (script/evaluation2.py:156-167)")


def _dist_stats(a: torch.Tensor, b: torch.Tensor) -> dict:
    a, b = a.detach().double().cpu().flatten(), b.detach().double().cpu().flatten()
    d = (a - b).abs()
    return dict(max_abs=float(d.max()), mean_abs=float(d.mean()),
                cosine=round(float((a * b).sum() / (a.norm() * b.norm())), 6))


def parity_report(mode: str, mine: torch.Tensor, ref: torch.Tensor, points: dict | None = None) -> dict:
    """Encoder-output distance of the TIMED graph's own output (image 0 of the last timed replay,
    fp32) from the oracle fed the same weights, scales and image, plus the mask IoU.

    int8 modes: ``points`` (``int8_reference_points``) carry the oracle's own fp64-vs-fp32 distance
    (max-abs, cosine, mask IoU) and, for W4A8, the int8 activation noise; ``pass`` is then gated
    against them (W8A8: cosine >= 0.995 and mask IoU mean >= the fp64 self mean - 0.02; W4A8:
    max-abs <= 1.5x the int8 noise, tests/test_w4a8.py:185, and the same mask IoU rule)."""
    mine = mine.detach().float()
    ref = ref.float()
    st = _dist_stats(mine, ref)
    rec = {"image": 0, "source": "the timed HIP graph's own output buffer (image 0 of the last timed replay)",
           "max_abs_vs_oracle": st["max_abs"], "mean_abs": st["mean_abs"], "ref_absmax": float(ref.abs().max())}
    try:
        rec.update(mask_iou_report(mine.reshape(1, 256, 64, 64), ref))
    except Exception as e:   # the report must not cost the throughput line
        rec["mask_iou_error"] = repr(e)[:200]
    iou_ok = None
    if points:
        refp = {}
        for k, v in points.items():
            r = _dist_stats(v, ref)
            try:
                m = mask_iou_report(v.float().reshape(1, 256, 64, 64), ref)
                r.update(mask_iou_min=m["mask_iou_min"], mask_iou_mean=m["mask_iou_mean"])
            except Exception as e:  # noqa: BLE001
                r["mask_iou_error"] = repr(e)[:200]
            refp[k] = r
        rec["reference_points"] = dict(refp, note="distance of each reference output from the fp32 oracle, "
                                       "same image / weights / scales: fp64 = the oracle's own graph in float64 "
                                       "(its self-distance), int8_noise = the graph without activation quantisers")
        selfp = refp.get("fp64", {})
        if "mask_iou_mean" in selfp and "mask_iou_mean" in rec:
            iou_ok = bool(rec["mask_iou_mean"] >= selfp["mask_iou_mean"] - 0.02)
    if mode == "w4a16":
        rec.update(oracle="G1 (oracle/sam_ref.py: fp32 encoder, GPTQ weights s*(q-zp))", tolerance=1e-2,
                   **{"pass": bool(st["max_abs"] <= 1e-2)})
    elif mode == "w4a8":
        rec.update(oracle="W4A8 composition (oracle/w4a8_ref.py) with the engine's calibrated activation scales")
        noise = (points or {}).get("int8_noise")
        if noise is not None:
            nmax = rec["reference_points"]["int8_noise"]["max_abs"]
            ok = st["max_abs"] <= 1.5 * nmax and iou_ok is not False
            rec.update(tolerance=f"max-abs <= 1.5 x int8 noise ({1.5 * nmax:.4f}; tests/test_w4a8.py:185) and mask "
                                 "IoU mean >= fp64 self mean - 0.02", **{"pass": bool(ok)})
        else:
            rec.update(tolerance="max-abs <= 0.35 (tests/test_w4a8.py:186)", **{"pass": bool(st["max_abs"] <= 0.35)})
    else:
        ok = st["cosine"] >= 0.995 and iou_ok is not False
        rec.update(oracle="fq_vit W8A8 fake-quant graph (oracle/fq_ref.py) with the engine's weights and calibrated "
                          "activation scales", cosine=st["cosine"],
                   tolerance="cosine >= 0.995 (tests/test_w8a8.py::test_w8a8_encoder_vs_golden)"
                             + (" and mask IoU mean >= fp64 self mean - 0.02" if iou_ok is not None else ""),
                   **{"pass": bool(ok)})
    return rec


def _state_shapes(cfg):
    shapes = {}
    c, heads = cfg["embed_dim"], cfg["num_heads"]
    hd = c // heads
    grid = cfg["img_size"] // 16
    shapes["patch_embed.proj.weight"] = (c, 3, 16, 16)
    shapes["patch_embed.proj.bias"] = (c,)
    shapes["pos_embed"] = (1, grid, grid, c)
    for i in range(cfg["depth"]):
        pre = f"blocks.{i}."
        side = grid if i in cfg["global_attn_indexes"] else 14
        for n, s in (("norm1.weight", (c,)), ("norm1.bias", (c,)), ("attn.qkv.weight", (3 * c, c)),
                     ("attn.qkv.bias", (3 * c,)), ("attn.proj.weight", (c, c)), ("attn.proj.bias", (c,)),
                     ("attn.rel_pos_h", (2 * side - 1, hd)), ("attn.rel_pos_w", (2 * side - 1, hd)),
                     ("norm2.weight", (c,)), ("norm2.bias", (c,)), ("mlp.lin1.weight", (4 * c, c)),
                     ("mlp.lin1.bias", (4 * c,)), ("mlp.lin2.weight", (c, 4 * c)), ("mlp.lin2.bias", (c,))):
            shapes[pre + n] = s
    shapes.update({"neck.0.weight": (256, c, 1, 1), "neck.1.weight": (256,), "neck.1.bias": (256,),
                   "neck.2.weight": (256, 256, 3, 3), "neck.3.weight": (256,), "neck.3.bias": (256,)})
    return shapes


def _cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def free_port() -> int:
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def launch_ranks(args, argv) -> int:
    """``--gpus N`` without a torchrun environment: start N fresh rank processes through
    ``torch.distributed.run`` as a child (nothing in this process has touched the GPU), let rank 0
    print the JSON line on the inherited stdout, and return the child's exit status."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()), str(Path(__file__).resolve()), *argv]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "4")
    log(f"launching {args.gpus} ranks: {' '.join(cmd[1:6])} ...")
    return subprocess.run(cmd, env=env).returncode


def local_images(start: int, stop: int, dev, dtype, size: int = 1024) -> torch.Tensor:
    """Images [start, stop) of the seeded global batch: image i ~ N(0, 1) from seed 1234 + i, so
    every sharding of the global batch sees the same pixels."""
    out = torch.empty((stop - start, 3, size, size), dtype=dtype, device=dev)
    for j, i in enumerate(range(start, stop)):
        g = torch.Generator(device=dev).manual_seed(1234 + i)
        out[j] = torch.randn((3, size, size), generator=g, device=dev, dtype=torch.float32).to(dtype)
    return out


DUMP_LIMIT_BYTES = 64 * 1000 * 1000


def dump_outputs(directory, arrays: dict) -> None:
    """``--dump-outputs``: write what the timed path returned in its last timed step as
    ``<directory>/<name>.npy`` (float32; float64 stays float64), at most 64 MB in all.  An array
    over its share of the limit is stored as a fixed sample: the flat elements at sorted indices
    drawn from seed 0, so two builds run with the same arguments store the same elements."""
    import numpy as np
    d = Path(directory)
    d.mkdir(parents=True, exist_ok=True)
    share = DUMP_LIMIT_BYTES // max(len(arrays), 1)
    for name, t in arrays.items():
        t = t.detach()
        t = t.double() if t.dtype == torch.float64 else t.float()
        keep = (share - 1024) // t.element_size()   # 1 KiB left for the .npy header
        if t.numel() > keep:
            g = torch.Generator(device="cpu").manual_seed(0)
            idx = torch.randint(t.numel(), (keep,), generator=g).sort().values
            t = t.flatten()[idx.to(t.device)]
        np.save(d / f"{name}.npy", t.cpu().numpy())


def dry_run(args, rank: int, world: int) -> None:
    """CPU rehearsal of the multi-rank path (gloo): shard the seeded global batch, broadcast a
    tiny quantised encoder from rank 0, gather per-rank shard / checksum records on rank 0."""
    from samq import dist as sdist
    from samq.synthetic import random_quant_encoder
    per_gpu = args.batch or 8
    gb = per_gpu * world
    start, stop = sdist.shard(gb, rank, world)
    imgs = local_images(start, stop, torch.device("cpu"), torch.float32, size=32)
    enc = random_quant_encoder("vit_b", -1, device="cpu", depth=1, img_size=64, init=(rank == 0))
    t_init = sdist.warm_up_collective()
    t0 = time.perf_counter()
    nbytes = sdist.broadcast_state(enc, src=0)
    t_bc = time.perf_counter() - t0
    wsum = float(sum(t.double().sum() for t in enc.state_dict().values() if torch.is_tensor(t)))
    rec = dict(rank=rank, shard=[start, stop], image_checksums=[float(x.double().sum()) for x in imgs],
               state_checksum=wsum, broadcast_bytes=nbytes, broadcast_s=round(t_bc, 4),
               first_collective_s=round(t_init, 4))
    on = dist.is_initialized()
    recs = [None] * world
    if on:
        dist.all_gather_object(recs, rec)
    else:
        recs = [rec]
    if rank == 0:
        print(json.dumps({"metric": METRIC, "value": None, "unit": "img/s", "n_gpus": world, "dry_run": True,
                          "backend": dist.get_backend() if on else None,
                          "world_size_seen": dist.get_world_size() if on else 1,
                          "global_batch": gb, "per_gpu_batch": per_gpu, "ranks": recs}), flush=True)
    if on:
        dist.barrier()
        dist.destroy_process_group()


def build_mode(mode: str, model: str, groupsize: int, rank: int, dev):
    """The mode's encoder on this rank: W4A16 / W4A8 random-init ViT-H RTN-packed on rank 0 and
    RCCL-broadcast (W4A8 then calibrates its activation quantisers on one seeded image); W8A8 a
    random-init fq_vit encoder calibrated on one seeded image (identical on every rank)."""
    import samq
    from samq import dist as sdist
    from samq.synthetic import random_fq_encoder, random_quant_encoder
    t_bc = 0.0
    if mode == "w8a8":
        return random_fq_encoder(model, device=dev), 0, 0.0, 0.0
    # model.half() as the reference's entry point runs it (gptq4sam_infer.py:59-79): the fp16
    # parameter values are what the engine and the parity oracle both see
    enc = random_quant_encoder(model, groupsize, device=dev, init=(rank == 0)).half()
    torch.cuda.synchronize()
    # the first collective creates the communicator (RCCL set-up) and waits for the slowest rank's
    # model build: timed on its own, so the broadcast time below is the transfer alone
    t_init = sdist.warm_up_collective(dev)
    tb = time.perf_counter()
    nbytes = sdist.broadcast_state(enc, src=0)
    torch.cuda.synchronize()
    t_bc = time.perf_counter() - tb
    if mode == "w4a8":
        samq.make_act_quant(enc)
        gcal = torch.Generator(device="cpu").manual_seed(99)
        cal = torch.randn((1, 3, 1024, 1024), generator=gcal).to(dev, torch.float16)
        samq.calibrate_act_quant(enc, enc.module_forward, [cal])
    return enc, nbytes, t_bc, t_init


def run_mode(mode: str, args, rank: int, world: int, dev, batch: int, lanes: int, *, headline: bool):
    """Build, capture and time one mode (``steps`` graph replays between barriers + synchronize,
    max over ranks), then -- outside the timed region -- its roofline, CPU baseline and parity.
    Returns the record (rank 0) or None."""
    from samq import dist as sdist
    from samq.synthetic import flops_per_image
    model = (args.model if headline else "") or ("vit_b" if mode == "w8a8" else "vit_h")
    groupsize = args.groupsize if (headline and mode == "w4a16") else -1
    t0 = time.time()
    enc, nbytes, t_bc, t_init = build_mode(mode, model, groupsize, rank, dev)
    eng = enc.engine()
    if headline and args.fold_ln:
        eng.fold_ln = True
    if headline and args.lane_stagger is not None:
        eng.lane_stagger = args.lane_stagger
    log(f"[rank {rank}] {mode} model ready in {time.time() - t0:.1f}s (broadcast {nbytes / 1e6:.1f} MB "
        f"in {t_bc * 1e3:.1f} ms after a {t_init * 1e3:.1f} ms first collective)")

    gb = world * batch
    start, stop = sdist.shard(gb, rank, world)
    img = local_images(start, stop, dev, torch.float32 if mode == "w8a8" else torch.float16)

    # the timed graph writes an fp32 encoder output (the parity stanza reads image 0 of it)
    if mode == "w8a8":
        fwd = (lambda: eng(img))   # noqa: E731
        cap = (lambda: eng.capture(img))   # noqa: E731
    else:
        fwd = (lambda: eng(img, out_dtype=torch.float32, lanes=lanes))   # noqa: E731
        cap = (lambda: eng.capture(img, out_dtype=torch.float32, lanes=lanes))   # noqa: E731
    holder = {}
    if args.no_graph:
        def run():
            holder["out"] = fwd()
    else:
        graph, holder["out"] = cap()
        run = graph.replay
    steps, warmup = args.steps, args.warmup
    for _ in range(warmup):
        run()
    torch.cuda.synchronize()
    on = dist.is_available() and dist.is_initialized()   # also a forced one-rank RCCL group
    if on:
        dist.barrier()
    torch.cuda.synchronize()
    rtx = _roctx()   # marks the timed window for tools/instep_profile.sh (no-op unprofiled)
    if rtx:
        rtx.roctxRangePushA(b"samq_timed_steps" if headline else f"samq_timed_steps_{mode}".encode())
    t_start = time.perf_counter()
    for _ in range(steps):
        run()
    torch.cuda.synchronize()
    if rtx:
        rtx.roctxRangePop()
    if on:
        dist.barrier()
    elapsed = time.perf_counter() - t_start
    if on:
        t = torch.tensor([elapsed, t_bc, t_init], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed, t_bc_max, t_init_max = t.tolist()
    else:
        t_bc_max, t_init_max = t_bc, t_init
    out0 = holder["out"][0:1].float().clone() if stop > start else None
    if headline and args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {"image_embeddings": holder["out"]})

    rows = stop - start
    per_launch_imgs = rows // lanes
    peak = PEAK_FP16_TFLOPS if mode == "w4a16" else PEAK_INT8_TOPS
    # (1) live, isolated: every GEMM launch of one forward at the lane's size, HIP events on the
    # launch stream, back to back
    iso = (dict(achieved=None, frac=None, avg_launch_us=None, launches_timed=0) if args.no_isolated else
           {"w4a16": gemm_roofline, "w4a8": w4a8_roofline, "w8a8": w8a8_roofline}[mode](eng, per_launch_imgs))
    # algorithmic bytes per GEMM launch: A once, packed W once, the output (fp32 residual = read +
    # write) once -- per mode: (A bytes/elem, W bytes/elem, out bytes/elem per layer)
    trows = per_launch_imgs * (eng.enc.img_size // eng.patch) ** 2 if mode == "w8a8" else per_launch_imgs * 4096
    a_b, w_b, outs = {"w4a16": (2, 0.5, (2, 8, 2, 8)), "w4a8": (1, 0.5, (2, 8, 1, 8)),
                      "w8a8": (1, 1, (1, 2, 1, 2))}[mode]
    alg = []
    for kn in gemm_shapes(mode, eng):
        for (k, n), out_b in zip(kn, outs):
            alg.append(trows * k * a_b + k * n * w_b + trows * n * out_b)
    alg_b = round(sum(alg) / len(alg))
    profile = PMC_PROFILES.get((mode, trows))
    traffic, src = pmc_traffic(mode, profile) if profile else (None, None)
    kernel = {"w4a16": "w4a16_gemm_pp2 (32x32x16 MFMA for qkv / lin1, 16x16x32 for proj / lin2): all 4 ViT-H "
                       "projection shapes",
              "w4a8": "i8_gemm_pp2 (int4 x int8 MFMA, zero point through row sums): all 4 ViT-H projection shapes",
              "w8a8": "i8_gemm_kernel W8 (int8 x int8 MFMA, vit_b projection shapes)"}[mode]
    flops_step = gemm_flops_per_step(mode, eng, rows)
    live = dict(achieved=iso["achieved"], frac=iso["frac"], avg_launch_us=iso["avg_launch_us"],
                launches_timed=iso["launches_timed"],
                method="HIP events on the launch stream around every GEMM launch of one forward at the lane's "
                       "size, back to back with no concurrent lane (3 reps)")
    ins = in_step_from_profile(mode, per_launch_imgs, lanes, flops_step, peak, groupsize)
    head = ins if ins else live
    roof = dict(bound="mfma", achieved=head["achieved"], peak=peak, unit="TFLOP/s", frac=head["frac"],
                traffic=traffic, traffic_unit="bytes per launch (L2->fabric, PMC)", traffic_source=src,
                algorithmic_bytes_per_launch=alg_b, kernel=kernel, avg_launch_us=head["avg_launch_us"],
                images_per_launch=per_launch_imgs,
                source=("in-step: the committed rocprofv3 kernel stats of this command on this build "
                        f"({ins['source']})" if ins else "live isolated (no committed in-step profile for this build)"),
                in_step=ins, isolated=live)
    fl = flops_per_image(enc)
    value = gb * steps / elapsed
    if rank != 0:
        return None
    e2e_tflops = value / world * fl["total"] / 1e12
    rec = {
        "value": round(value, 3), "unit": "img/s", "n_gpus": world, "steps": steps, "warmup": warmup,
        "ms_per_step": round(elapsed / steps * 1e3, 3),
        "dtype": {"w4a16": "fp16", "w4a8": "int8", "w8a8": "int8"}[mode],
        "config": {"workload": {
            "w4a16": f"SAM {model} image encoder W4A16 GPTQ (int4 RTN-packed, groupsize {groupsize})",
            "w4a8": f"SAM {model} image encoder W4A8 (GPTQ int4 weights, int8 minmax activations)",
            "w8a8": f"SAM {model} image encoder W8A8 fq_vit (int8 per-channel weights, int8 activations)",
        }[mode] + f", {batch} x 1024x1024 images per GPU", "mode": mode,
                   "model": model, "global_batch": gb, "per_gpu_batch": batch,
                   "seq_len": 4096, "parallelism": f"image-parallel x{world} (weights RCCL-broadcast once)",
                   "graph": not args.no_graph, "lanes": lanes, "groupsize": groupsize},
        "roofline": roof,
        "e2e": {"tflop_per_image": round(fl["total"] / 1e12, 4), "achieved_tflops_per_gpu": round(e2e_tflops, 1),
                "frac_of_fp16_peak": round(e2e_tflops / PEAK_FP16_TFLOPS, 4),
                "frac_of_int8_peak": round(e2e_tflops / (2 * PEAK_FP16_TFLOPS), 4)},
        "dist": {"backend": dist.get_backend() if on else None, "world_size_seen": world,
                 "broadcast_bytes": nbytes, "broadcast_ms": round(t_bc_max * 1e3, 2),
                 "broadcast_GBps": round(nbytes / t_bc_max / 1e9, 2) if nbytes and t_bc_max > 0 else None,
                 "first_collective_ms": round(t_init_max * 1e3, 2),
                 "broadcast_method": "max over ranks; timed after a one-element all_reduce that creates the "
                                     "communicator and waits for rank 0's model build (first_collective_ms)",
                 "rank0_shard": [start, stop]},
        "parity": None, "cpu_baseline": None,
    }
    if not args.no_cpu_baseline and out0 is not None:
        # checker leg, after the timed region: the oracle fed this encoder's weights and rank 0's
        # image 0 (= global image 0 at every N); the CPU baseline is timed at N = 1 only, and the
        # other ranks wait at the final barrier meanwhile
        if world == 1:
            rec["cpu_baseline"], ref = cpu_baseline(model, mode, enc, img[0], groupsize)
        else:
            ref = parity_reference(model, mode, enc, img[0], groupsize)
        points = int8_reference_points(model, mode, enc, img[0], groupsize) if mode != "w4a16" else None
        rec["parity"] = parity_report(mode, out0, ref, points)
    del eng, enc, img, holder
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=0, help="images per GPU (default 4 at N=1, 8 at N>1)")
    ap.add_argument("--model", default="")
    ap.add_argument("--mode", default="w4a16", choices=("w4a16", "w4a8", "w8a8"))
    ap.add_argument("--groupsize", type=int, default=-1)
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--lanes", type=int, default=0,
                    help="image groups run as concurrent kernel chains on separate HIP streams "
                         "(0 = 2 when the per-GPU batch is even, else 1; W8A8 runs one chain)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also measure and check everything else: the isolated GEMM "
                         "roofline passes, the CPU baseline, parity + mask IoU of the timed output against the "
                         "oracle, and (1-GPU W4A16) the W4A8 / W8A8 sub-records; without it a run sets up, warms "
                         "up, times the steps and prints the line")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="after the timed steps write rank 0's encoder output of the last timed step to "
                         "DIR/image_embeddings.npy (float32; a seeded sample above 64 MB)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-modes", action="store_true",
                    help="headline only: skip the W4A8 (config 5) / W8A8 (config 2) sub-records that a --full "
                         "1-GPU W4A16 run appends")
    ap.add_argument("--lane-stagger", type=int, default=None,
                    help="W4A16 lanes: lane i+1 waits for lane i's launch k (7 per block; -1 = none; default: the engine's 1)")
    ap.add_argument("--fold-ln", action="store_true",
                    help="W4A16: fold the LayerNorms into the GEMM epilogues (opt-in A/B; measured slower)")
    ap.add_argument("--no-isolated", action="store_true",
                    help="skip the live roofline passes (for a rocprof trace of the timed replays only)")
    ap.add_argument("--backend", default="", help="torch.distributed backend (default nccl = RCCL; gloo for --dry-run)")
    ap.add_argument("--dry-run", action="store_true", help="CPU rehearsal of the multi-rank path (no GPU)")
    argv = sys.argv[1:]
    args = ap.parse_args(argv)
    if not args.full:   # a plain run: the headline alone (the --no-* switches trim a --full run)
        args.no_cpu_baseline = args.no_isolated = args.no_modes = True

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(launch_ranks(args, argv))

    from samq import dist as sdist
    rank, world = sdist.init_from_env(args.backend or ("gloo" if args.dry_run else None))
    if world != args.gpus:
        log(f"warning: --gpus {args.gpus} but WORLD_SIZE={world}; using {world}")
    if args.dry_run:
        return dry_run(args, rank, world)

    # one GPU per local rank; more ranks than GPUs only for a gloo rehearsal of the N-rank path on a
    # smaller box (ranks then share the GPUs round-robin) -- never silently under RCCL
    lr, ndev = int(os.environ.get("LOCAL_RANK", "0")), torch.cuda.device_count()
    if lr >= ndev and (dist.is_initialized() and dist.get_backend() != "gloo" or ndev == 0):
        raise SystemExit(f"LOCAL_RANK {lr} but only {ndev} visible GPUs: one rank per GPU (a shared-GPU "
                         "rehearsal needs --backend gloo)")
    dev = torch.device("cuda", lr % ndev)
    torch.cuda.set_device(dev)
    mode = args.mode
    batch = args.batch or default_batch(mode, world)
    if mode == "w8a8":
        if args.lanes > 1:
            ap.error("--mode w8a8 runs one kernel chain (W8A8Engine has no lanes)")
        args.lanes = 1
    elif args.lanes <= 0:
        args.lanes = default_lanes(mode, batch)
    if batch % args.lanes:
        ap.error(f"--lanes {args.lanes} does not divide the per-GPU batch {batch}")

    rec = run_mode(mode, args, rank, world, dev, batch, args.lanes, headline=True)
    modes = None
    if world == 1 and mode == "w4a16" and not args.no_modes and not args.no_cpu_baseline and args.groupsize == -1:
        # configs 5 and 2 measured in the same driver run, each with its own timed graph, roofline
        # (in-step profile of this build) and parity of its timed output
        modes = {}
        torch.cuda.empty_cache()
        for m in ("w4a8", "w8a8"):
            b = default_batch(m, world)
            margs = argparse.Namespace(**vars(args))
            if m == "w8a8":
                # a vit_b B=1 step is ~1.8 ms: 20 steps are a 35 ms window, short enough for the
                # first replays' clock ramp to bias it (20 / 5 steps 577-581 vs 200 / 50 steps 593
                # img/s on one box); the sub-record times >= 200 steps after >= 50 warm-up steps and
                # reports the counts it used
                margs.steps, margs.warmup = max(args.steps, 200), max(args.warmup, 50)
            try:   # a sub-mode failure is reported in the line; it never costs the headline record
                modes[m] = run_mode(m, margs, rank, world, dev, b, default_lanes(m, b), headline=False)
            except Exception as e:  # noqa: BLE001
                log(f"mode {m} failed: {type(e).__name__}: {e}")
                modes[m] = {"error": f"{type(e).__name__}: {e}"}
            torch.cuda.empty_cache()
    if rank == 0:
        line = {"metric": METRIC, "value": rec.pop("value"), "unit": rec.pop("unit"), "n_gpus": world,
                "steps": rec.pop("steps"), "warmup": rec.pop("warmup"), "ms_per_step": rec.pop("ms_per_step"),
                "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": rec.pop("dtype"),
                "data": "synthetic"}
        line.update(rec)
        if modes is not None:
            line["modes"] = modes
        print(json.dumps(line), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def default_batch(mode: str, world: int) -> int:
    """BASELINE configs: W4A16 4 images per GPU at N=1 (config 3), 8 at N>1 (config 4 at N=8 =
    global batch 64); W4A8 8 (config 5); W8A8 1 (config 2)."""
    return {"w4a16": 4 if world == 1 else 8, "w4a8": 8, "w8a8": 1}[mode]


def default_lanes(mode: str, batch: int) -> int:
    # W4A16: two images per lane (M = 8192 per GEMM launch, the size the tile picks and the quoted
    # roofline are tuned on; B=8 on 4 lanes 48.30 vs 49.02 ms on 2, tools/bench_lanes.py); W4A8 two
    # lanes; W8A8 one chain
    if mode == "w8a8":
        return 1
    return (batch // 2 if mode == "w4a16" else 2) if batch % 2 == 0 else 1


if __name__ == "__main__":
    main()
