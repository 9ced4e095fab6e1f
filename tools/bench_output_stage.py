#!/usr/bin/env python
"""Cost of the tester's output stage, host route against device route (patchrefinerv2_amd/output.py).  One JSON line.

    python tools/bench_output_stage.py [--workload v2_zoe_4k_r32] [--frames 3] [--workers 8] [--prec f16f6] [--skip-model] [--runs N]

Per resolution (1080p, 4K), on one synthetic depth map:
  host_stage_ms      the host stage of Tester._emit (16-bit PNG, colour PNG, edge PNG), median of 3
  device_kernels_ms  the device kernels of OutputStage.submit_frame's files, HIP events after a warm-up, median of 20
  d2h_bytes_*        bytes copied device -> host per frame on either route (fp32 map / packed scanlines)
  deflate            per file kind (16-bit depth, colour, edge mask): the device encoder's kernel ms (HIP events, median of 10), its
                     stream size, and len(zlib.compress(rows, 1)) / len(zlib.compress(rows, 6)) of the same scanlines
Then Tester.run(save=True) and Tester.generate_pl(save=True) maps/s on the workload (synthetic weights): no save, host route,
device route, device route with --device-deflate, over ``--frames`` frames each (wall clock around the whole call, files on disk
when it returns), and the bytes copied device -> host per frame on the two device routes (d2h_bytes_per_frame_*).  ``--runs N``
repeats the rate measurements N times on the one model: every rate is then the median, with [min, max] under "min_max".
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def synth_depth(h, w, seed=0):
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    rs = np.random.RandomState(seed)
    d = 5.0 + 30.0 * (x / w) + 8.0 * (np.hypot(x - w * 0.6, y - h * 0.5) < h * 0.2) + 4.0 * np.sin(y / 37.0) + 0.05 * rs.rand(h, w)
    return d.astype(np.float32)


def stage_costs(h, w, tmp):
    from patchrefinerv2_amd import metrics as M, ops
    from patchrefinerv2_amd.output import colorize_device
    from patchrefinerv2_amd.tester import write_png8, write_png16
    d = synth_depth(h, w)
    t = torch.from_numpy(d)

    def host():
        write_png16(os.path.join(tmp, "h_uint16.png"), (t.squeeze().numpy() * 256).astype("uint16"))
        write_png8(os.path.join(tmp, "h.png"), np.ascontiguousarray(M.colorize(t, cmap="Spectral", vminp=0, vmaxp=100)[:, :, :3]))
        write_png8(os.path.join(tmp, "h_edge.png"), M.depth_edges(t).astype(np.uint8) * 255)

    host_ms = []
    for _ in range(3):
        t0 = time.perf_counter()
        host()
        host_ms.append(1000.0 * (time.perf_counter() - t0))
    dev = torch.from_numpy(d).cuda()[None]

    def device():
        rows = [ops.quantize16_rows(dev, 256.0), colorize_device(dev[0], cmap="Spectral", vminp=0, vmaxp=100)[1],
                ops.mask_rows(ops.binary_dilate(ops.canny(ops.depth_preprocess(dev, "log"), sigma=1.0), 3))]
        return sum(int(r.shape[1]) for r in rows)

    for _ in range(3):
        packed = device()
    ms = []
    for _ in range(20):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        device()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    import zlib
    kinds = dict(depth16=(2, lambda: ops.quantize16_rows(dev, 256.0)), colour=(3, lambda: colorize_device(dev[0], cmap="Spectral", vminp=0, vmaxp=100)[1]),
                 mask=(1, lambda: ops.mask_rows(ops.binary_dilate(ops.canny(ops.depth_preprocess(dev, "log"), sigma=1.0), 3))))
    deflate = {}
    for kind, (bpp, make) in kinds.items():
        rows, n = make(), h * (1 + bpp * w)
        for _ in range(2):
            out, nb = ops.deflate_rows(rows, n)
        dms = []
        for _ in range(10):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            out, nb = ops.deflate_rows(rows, n)
            e1.record()
            torch.cuda.synchronize()
            dms.append(e0.elapsed_time(e1))
        raw = rows[0, :n].cpu().numpy().tobytes()
        assert zlib.decompress(out[0, :int(nb[0])].cpu().numpy().tobytes()) == raw
        deflate[kind] = dict(bytes=n, deflate_kernels_ms=round(statistics.median(dms), 3), stream_bytes=int(nb[0]),
                             zlib1_bytes=len(zlib.compress(raw, 1)), zlib6_bytes=len(zlib.compress(raw, 6)))
    return dict(host_stage_ms=round(statistics.median(host_ms), 1), device_kernels_ms=round(statistics.median(ms), 3),
                d2h_bytes_host=h * w * 4, d2h_bytes_device=packed, deflate=deflate)


def tester_rates(args, tmp):
    from patchrefinerv2_amd import models, weights as W  # noqa: F401
    from patchrefinerv2_amd.registry import build_model
    from patchrefinerv2_amd.tester import ImageDataset, RunnerInfo, Tester
    from patchrefinerv2_amd.workloads import WORKLOADS, model_config, state_spec
    w = WORKLOADS[args.workload]
    model = build_model(model_config(args.workload, prec=args.prec, max_batch=int(w.get("max_batch", 41)), n_streams=3))
    model.load_state_dict(W.synth_state_dict(state_spec(args.workload), seed=0), strict=True)
    imgs = os.path.join(tmp, "imgs")
    os.makedirs(imgs)
    for i in range(args.frames):
        np.save(os.path.join(imgs, f"f{i}.npy"), np.random.RandomState(i).rand(270, 480, 3).astype(np.float32))
    ds = ImageDataset(imgs, image_resolution=w["raw"])
    samples, out = {}, {}
    routes = ("warmup", "no_save", "host", "device", "device_deflate")
    for rep in range(max(1, args.runs)):
        for kind in ("run", "generate_pl"):
            for route in routes if rep == 0 else routes[1:]:
                info = RunnerInfo(save=route in ("host", "device", "device_deflate"), device_output=route in ("device", "device_deflate"),
                                  device_deflate=route == "device_deflate", output_workers=args.workers, work_dir=os.path.join(tmp, f"{kind}_{route}"))
                t = Tester(None, info, ds, model)
                kw = dict(cai_mode=w["mode"], image_raw_shape=w["raw"], patch_split_num=w["split"], seed=621)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                t.run(**kw) if kind == "run" else t.generate_pl(**kw)
                torch.cuda.synchronize()
                if route != "warmup":
                    samples.setdefault(f"{kind}_{route}_maps_per_s", []).append(round(args.frames / (time.perf_counter() - t0), 3))
                if route in ("device", "device_deflate"):
                    out[f"{kind}_d2h_bytes_per_frame_{route}"] = t.last_output_stage.bytes_d2h // args.frames
    for k, v in samples.items():
        out[k] = round(statistics.median(v), 3)
    if args.runs > 1:
        out["runs"] = args.runs
        out["min_max"] = {k: [min(v), max(v)] for k, v in samples.items()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="v2_zoe_4k_r32")
    ap.add_argument("--frames", type=int, default=3)
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--prec", default="f16f6", choices=["f32", "bf16x3", "f16f6"])
    ap.add_argument("--skip-model", action="store_true", help="the stage costs only")
    ap.add_argument("--runs", type=int, default=1, help="repeat the rate measurements: medians, with [min, max] under min_max")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    res = dict(workload=args.workload, prec=args.prec, frames=args.frames, workers=args.workers)
    with tempfile.TemporaryDirectory() as tmp:
        res["1080p"] = stage_costs(1080, 1920, tmp)
        res["4k"] = stage_costs(2160, 3840, tmp)
        if not args.skip_model:
            res.update(tester_rates(args, tmp))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
