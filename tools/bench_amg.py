#!/usr/bin/env python3
"""The automatic mask generator's two irregular steps per call: ``ops.mask_rle`` and ``ops.box_nms`` against
plain-torch compositions written for this tool.

    python tools/bench_amg.py [--reps 7] [--out amg.jsonl]

RLE: 192 blob-like masks (smooth low-res logits: seeded 8 x 8 noise upsampled to 256 x 256, through
``ops.mask_postprocess``) at 1024 x 1024, 683 x 1024 and 1200 x 1800, of which about 10 %, 50 % and 100 % are
selected.  The torch composition is the upstream recipe without its pad: the masks are the whole canvas here
(no crop), where the upstream uncrop step hands them on as they are, so it starts at the permute to Fortran
order, then xor of neighbours, ``nonzero``, and per mask a boolean split and a host transfer.  NMS: n = 192, 3072 and 12288 boxes
clustered around 40 centres, seeded scores, threshold 0.7, against a greedy loop on the device (one row of IoUs
per kept box).  The two paths alternate ``--reps`` times after a warm-up of each; a timed run is ``inner``
back-to-back calls on the host clock between device synchronisations, ``inner`` chosen so a run lasts about 20 ms
or more.  One JSON line per point: medians per call in ms, min / max of the runs, whether the two paths agree
and, for the RLE, the HBM bound of two reads of the selected masks at 8 TB/s and the HIP path's share of it.

Small regions (``--only regions``): ``ops.rle_remove_small_regions`` with ``min_area`` 100 on the run lengths of all
192 blob masks at the three sizes, with the segments per mask, against the upstream host composition per mask
(decode, connected components twice, box, re-encode) where the host has OpenCV or, failing that,
``scipy.ndimage``; the ``host`` field says which, ``null`` and no comparison if neither.

Whole generator (``--only generate``): ``SamAutomaticMaskGenerator.generate`` with ``crop_n_layers=1`` (five crops,
8 x 8 points each, no score filters) on a 1200 x 1800 image and a W4A16 vit_b with random weights: every crop
resized from the resident image (``hip``) against ``set_image`` replaced by the host steps it took before
``ops.resize_u8`` (``host``: slice, PIL resize, upload per crop), and whether the two give equal records.
``--fused-tail on`` runs it with the float mask decoder's fused tail; ``--only generate_tail`` alternates the same
``generate`` with the tail as the module graph (``module``) and as the two HIP launches (``hip``).
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "sam-quantization_amd"))

import torch  # noqa: E402

HBM_BYTES_PER_S = 8e12


def torch_rle(masks, sel):
    """mask_to_rle_pytorch on masks[sel]: a list of run-length lists."""
    m = masks[sel]
    b, h, w = m.shape
    t = m.permute(0, 2, 1).flatten(1)
    idx = (t[:, 1:] ^ t[:, :-1]).nonzero()
    first = t[:, 0].cpu().tolist()
    out = []
    for i in range(b):
        cur = idx[idx[:, 0] == i, 1] + 1
        ends = torch.cat([cur.new_zeros(1), cur, cur.new_full((1,), h * w)])
        runs = (ends[1:] - ends[:-1]).cpu().tolist()
        out.append(([0] if first[i] else []) + runs)
    return out


def torch_nms(boxes, scores, thr):
    order = torch.sort(scores, stable=True, descending=True).indices
    b = boxes[order]
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    dead = torch.zeros(len(b), dtype=torch.bool, device=b.device)
    keep = []
    for i in range(len(b)):
        if dead[i]:
            continue
        keep.append(i)
        w = (torch.minimum(b[i, 2], b[i + 1:, 2]) - torch.maximum(b[i, 0], b[i + 1:, 0])).clamp(min=0)
        h = (torch.minimum(b[i, 3], b[i + 1:, 3]) - torch.maximum(b[i, 1], b[i + 1:, 1])).clamp(min=0)
        dead[i + 1:] |= w * h / (area[i] + area[i + 1:] - w * h) > thr
    return order[torch.tensor(keep, device=b.device)]


def timed(fn, inner):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / inner * 1e3, out


def compare(paths, reps):
    inner, t, out = {}, {k: [] for k in paths}, {}
    for name, fn in paths.items():
        timed(fn, 1)
        inner[name] = max(1, min(200, int(20.0 / max(timed(fn, 1)[0], 1e-3))))
    for _ in range(reps):
        for name, fn in paths.items():
            dt, out[name] = timed(fn, inner[name])
            t[name].append(dt)
    res = {"inner": inner}
    for k, v in t.items():
        res[f"{k}_ms"] = round(statistics.median(v), 4)
        res[f"{k}_min_max_ms"] = [round(min(v), 4), round(max(v), 4)]
    other = next((k for k in paths if k != "hip"), None)
    if other is not None:
        res["speedup"] = round(res[f"{other}_ms"] / res["hip_ms"], 2)
    return res, out


def rle_point(orig, frac, reps, dev):
    from samq import ops
    from samq.sam_decoder import ResizeLongestSide
    g = torch.Generator(device="cpu").manual_seed(orig[0] + orig[1])
    low = torch.nn.functional.interpolate(3 * torch.randn((192, 1, 8, 8), generator=g) - 1.5, (256, 256),
                                          mode="bicubic")[:, 0].contiguous().to(dev)
    inp = ResizeLongestSide.get_preprocess_shape(orig[0], orig[1], 1024)
    masks, _ = ops.mask_postprocess(low, 1024, inp, orig)
    n_sel = max(1, round(192 * frac))
    sel = torch.randperm(192, generator=g)[:n_sel].to(dev)
    res, out = compare({"torch": lambda: torch_rle(masks, sel), "hip": lambda: ops.mask_rle(masks, sel)}, reps)
    offsets, counts = (v.cpu() for v in out["hip"])
    same = [counts[offsets[i]:offsets[i + 1]].tolist() for i in range(n_sel)] == out["torch"]
    bound_ms = 2 * n_sel * orig[0] * orig[1] / HBM_BYTES_PER_S * 1e3
    return dict(op="mask_rle", size=list(orig), n_sel=n_sel, runs=int(offsets[-1]), **res,
                hbm_bound_ms=round(bound_ms, 5), hip_share_of_hbm_bound=round(bound_ms / res["hip_ms"], 4), equal=same)


def nms_point(n, reps, dev):
    from samq import ops
    g = torch.Generator(device="cpu").manual_seed(n)
    centre = 1024 * torch.rand((40, 2), generator=g)
    c = centre[torch.randint(0, 40, (n,), generator=g)] + 30 * torch.randn((n, 2), generator=g)
    half = 20 + 100 * torch.rand((n, 2), generator=g)
    boxes = torch.cat([c - half, c + half], 1).round().to(dev)
    scores = torch.rand(n, generator=g).to(dev)
    res, out = compare({"torch": lambda: torch_nms(boxes, scores, 0.7), "hip": lambda: ops.box_nms(boxes, scores, 0.7)},
                       reps)
    return dict(op="box_nms", n=n, kept=int(out["hip"].numel()), **res, equal=bool(torch.equal(out["hip"], out["torch"])))


def host_labeller():
    """(name, label function) of the host's connected components: OpenCV as the upstream step uses it, else
    scipy.ndimage with the 8-neighbour structure, else ``(None, None)``.  label(mask) -> (labels, areas incl. 0)."""
    try:
        import cv2
        return "cv2", lambda m: (lambda r: (r[1], r[2][:, -1]))(cv2.connectedComponentsWithStats(m.astype("uint8"), 8))
    except ImportError:
        pass
    try:
        import numpy as np
        from scipy import ndimage
        return "scipy.ndimage", lambda m: (lambda lab: (lab, np.bincount(lab.ravel())))(
            ndimage.label(m, structure=np.ones((3, 3), dtype=int))[0])
    except ImportError:
        return None, None


def host_regions(offsets, counts, size, min_area, label):
    """The upstream host composition per mask: decode, holes, islands, box, re-encode of the changed ones."""
    import numpy as np
    from samq.automatic_mask_generator import rle_to_mask
    offsets, counts = offsets.cpu().numpy(), counts.cpu().numpy()
    rows, boxes, same = [], [], []
    for i in range(len(offsets) - 1):
        row = counts[offsets[i]:offsets[i + 1]]
        mask = rle_to_mask({"size": list(size), "counts": row})
        changed = False
        for holes in (True, False):
            lab, areas = label(mask ^ holes)
            small = [k for k in range(1, len(areas)) if areas[k] < min_area]
            if not small:
                continue
            changed = True
            fill = [0] + small
            if not holes:
                fill = [k for k in range(len(areas)) if k not in fill] or [int(np.argmax(areas[1:])) + 1]
            mask = np.isin(lab, fill)
        ys, xs = np.nonzero(mask)
        boxes.append([xs.min(), ys.min(), xs.max(), ys.max()] if len(xs) else [0, 0, 0, 0])
        same.append(not changed)
        if changed:
            flat = mask.flatten(order="F")
            ends = np.concatenate([[0], np.flatnonzero(flat[1:] != flat[:-1]) + 1, [flat.size]])
            row = np.concatenate([[0] if flat[0] else [], np.diff(ends)]).astype(np.int32)
        rows.append(row)
    return rows, boxes, same


def regions_point(orig, reps, dev, min_area=100):
    from samq import ops
    from samq.sam_decoder import ResizeLongestSide
    g = torch.Generator(device="cpu").manual_seed(orig[0] + orig[1])
    low = torch.nn.functional.interpolate(3 * torch.randn((192, 1, 8, 8), generator=g) - 1.5, (256, 256),
                                          mode="bicubic")[:, 0].contiguous().to(dev)
    masks, _ = ops.mask_postprocess(low, 1024, ResizeLongestSide.get_preprocess_shape(orig[0], orig[1], 1024), orig)
    offsets, counts = ops.mask_rle(masks)
    segments = (masks[:, 1:] != masks[:, :-1]).sum((1, 2)) + orig[1]
    name, label = host_labeller()
    paths = {"hip": lambda: ops.rle_remove_small_regions(offsets, counts, orig, min_area)}
    if label is not None:
        paths["host"] = lambda: host_regions(offsets, counts, orig, min_area, label)
    res, out = compare(paths, reps)
    o, c, boxes, _, same = (v.cpu() for v in out["hip"])
    rec = dict(op="rle_remove_small_regions", size=list(orig), n=192, min_area=min_area, runs=int(offsets[-1]),
               segments_per_mask=round(float(segments.float().mean()), 1), segments_max=int(segments.max()),
               changed=int((~same).sum()), **res, host=name)
    if label is not None:
        rows, hboxes, hsame = out["host"]
        # a tie between the largest of all-small islands may go to another island on the host: see DESIGN.md
        rec["equal"] = (all(c[o[i]:o[i + 1]].tolist() == rows[i].tolist() for i in range(192))
                        and boxes.tolist() == [[int(v) for v in b] for b in hboxes] and same.tolist() == hsame)
    return rec


def generate_point(reps, dev, orig=(1200, 1800), fused_tail=False):
    import numpy as np
    import samq
    from samq.build_sam import Sam
    from samq.synthetic import random_quant_encoder
    torch.manual_seed(0)
    gen = samq.SamAutomaticMaskGenerator(Sam(random_quant_encoder("vit_b", device=dev)).to(dev).eval(),
                                         points_per_side=8, pred_iou_thresh=0.0, stability_score_thresh=0.0,
                                         crop_n_layers=1, output_mode="uncompressed_rle")
    gen.predictor.model.mask_decoder.use_fused_tail = fused_tail
    image = np.random.Generator(np.random.PCG64(1)).integers(0, 256, orig + (3,), dtype=np.uint8)
    pred, device_set_image = gen.predictor, gen.predictor.set_image

    def host_set_image(_, image_format="RGB", box=None):
        x0, y0, x1, y1 = box
        crop = image[y0:y1, x0:x1]
        inp = pred.transform.apply_image(np.ascontiguousarray(crop))
        pred.set_torch_image(torch.as_tensor(inp, device=dev).permute(2, 0, 1).contiguous()[None], crop.shape[:2])

    def run(set_image):
        pred.set_image = set_image
        return gen.generate(image)

    res, out = compare({"host": lambda: run(host_set_image), "hip": lambda: run(device_set_image)}, reps)
    return dict(op="generate", size=list(orig), crop_n_layers=1, fused_tail=fused_tail, records=len(out["hip"]), **res,
                equal=out["hip"] == out["host"])


def generate_tail_point(reps, dev, orig=(1200, 1800)):
    """One ``generate`` of the float decoder behind the GPTQ encoder, the decoder's tail as the module graph
    (``module``) against the two fused launches (``hip``: ``mask_decoder.use_fused_tail = True``), alternating."""
    import numpy as np
    import samq
    from samq.build_sam import Sam
    from samq.synthetic import random_quant_encoder
    torch.manual_seed(0)
    gen = samq.SamAutomaticMaskGenerator(Sam(random_quant_encoder("vit_b", device=dev)).to(dev).eval(),
                                         points_per_side=8, pred_iou_thresh=0.0, stability_score_thresh=0.0,
                                         crop_n_layers=1, output_mode="uncompressed_rle")
    image = np.random.Generator(np.random.PCG64(1)).integers(0, 256, orig + (3,), dtype=np.uint8)

    def run(fused):
        gen.predictor.model.mask_decoder.use_fused_tail = fused
        return gen.generate(image)

    res, out = compare({"module": lambda: run(False), "hip": lambda: run(True)}, reps)
    return dict(op="generate_tail", size=list(orig), crop_n_layers=1, records=len(out["hip"]),
                records_module=len(out["module"]), **res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="")
    ap.add_argument("--only", default="", choices=["", "mask_rle", "box_nms", "regions", "generate", "generate_tail"])
    ap.add_argument("--fused-tail", choices=["off", "on"], default="off",
                    help="the float mask decoder's tail in the other points: module graph (off) or the two HIP launches")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_amg: no GPU visible; timings are taken on the GPU only")
    dev = torch.device("cuda:0")
    name = torch.cuda.get_device_name(0)
    points = [lambda o=o, f=f: rle_point(o, f, a.reps, dev) for o in ((1024, 1024), (683, 1024), (1200, 1800))
              for f in (0.1, 0.5, 1.0)] + [lambda n=n: nms_point(n, a.reps, dev) for n in (192, 3072, 12288)]
    points += [lambda o=o: regions_point(o, a.reps, dev) for o in ((1024, 1024), (683, 1024), (1200, 1800))]
    points += [lambda: generate_point(a.reps, dev, fused_tail=a.fused_tail == "on"),
               lambda: generate_tail_point(a.reps, dev)]
    if a.only:
        ops_ = ["mask_rle"] * 9 + ["box_nms"] * 3 + ["regions"] * 3 + ["generate", "generate_tail"]
        points = [p for p, op in zip(points, ops_) if op == a.only]
    for p in points:
        line = json.dumps(dict(p(), reps=a.reps, device=name))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
