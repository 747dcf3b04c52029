"""What the train-time warp costs per batch: preprocess_batch with and without `augment` (one process, alternating), the
warp launch alone (HIP events over queued calls), the host cost of Augment.params, and the same warp by Pillow on the
host (the two calls torchvision makes for a PIL image, one core).

256 pages of bench.py's `--mode preprocess` shapes (30 - 119 x 80 - 779 pixels, L and RGB alternating) -> (256, 3, 64, 320).
The host figures (params, Pillow) need no GPU: `--host-only` times them alone.
usage: python profiles/augment_cost.py [--batches N] [--rounds R] [--host-only] [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "hmer-img2latex_amd"))
from img2latex_amd import synth                                                  # noqa: E402
from img2latex_amd.data import Augment                                           # noqa: E402


def make_pages(n):
    sizes = [(30 + (7 * k) % 90, 80 + (53 * k) % 700, 1 + 2 * (k % 2)) for k in range(n)]
    return [np.round(synth.uniform(5000 + k, "img", (h, w, c), 0.0, 255.0)).astype(np.uint8).reshape((h, w) if c == 1 else (h, w, 3))
            for k, (h, w, c) in enumerate(sizes)]


def pillow_batch(pages, angles, tx, ty):
    from PIL import Image
    out = []
    for p, a, x, y in zip(pages, angles, tx, ty):
        white = 255 if p.ndim == 2 else (255, 255, 255)
        rot = Image.fromarray(p).rotate(float(a), resample=Image.NEAREST, expand=False, center=None, fillcolor=white)
        out.append(np.asarray(rot.transform(rot.size, Image.AFFINE, (1, 0, -int(x), 0, 1, -int(y)), resample=Image.NEAREST,
                                            fillcolor=white)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment_cost.txt"))
    args = ap.parse_args()
    B = 256
    pages = make_pages(B)
    sizes = [p.shape[:2] for p in pages]
    aug = Augment(seed=1)
    ids = np.arange(B)
    lines = [f"augment_cost: {B} pages, {sum(p.size for p in pages) / 1e6:.1f} MB, {args.rounds} rounds", ""]

    t_params = []
    for r in range(max(args.rounds, 3)):
        t0 = time.perf_counter()
        for e in range(20):
            aug.params(sizes, ids, e)
        t_params.append((time.perf_counter() - t0) / 20 * 1e3)
    lines.append(f"Augment.params (host, one core): median {statistics.median(t_params):.3f} ms per batch "
                 f"(runs: {', '.join(f'{t:.3f}' for t in t_params)})")
    try:
        import PIL
        angles, tx, ty = aug.draw(sizes, ids, 0)
        t_pil = []
        for r in range(max(args.rounds, 3)):
            t0 = time.perf_counter()
            pillow_batch(pages, angles, tx, ty)
            t_pil.append((time.perf_counter() - t0) * 1e3)
        lines.append(f"the same warp by Pillow {PIL.__version__} (host, one core, arrays in and out): median "
                     f"{statistics.median(t_pil):.2f} ms per batch = {B / statistics.median(t_pil) * 1e3:.0f} images/s "
                     f"(runs: {', '.join(f'{t:.2f}' for t in t_pil)})")
    except ImportError:
        lines.append("Pillow is not installed: no host comparison")

    if not args.host_only:
        import torch
        from img2latex_amd import _lib
        from img2latex_amd.data import preprocess_batch
        from img2latex_amd.data.augment import PARAMS_DTYPE
        from img2latex_amd.data.preprocess import PLAN_DTYPE
        assert torch.cuda.is_available(), "the device figures need the MI355X (--host-only for the rest)"
        routes = {"preprocess_batch": lambda e: preprocess_batch(pages, (64, 320), 3, True),
                  "preprocess_batch(augment=...)": lambda e: preprocess_batch(pages, (64, 320), 3, True, augment=aug,
                                                                              sample_ids=ids, epoch=e)}
        for fn in routes.values():
            for e in range(10):
                fn(e)
        times = {k: [] for k in routes}
        for _ in range(args.rounds):
            for name, fn in routes.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for e in range(args.batches):
                    fn(e)
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) / args.batches * 1e3)
        for name, ts in times.items():
            lines.append(f"{name}: median {statistics.median(ts):.3f} ms per batch = {B / statistics.median(ts):.0f} k images/s "
                         f"(rounds: {', '.join(f'{t:.3f}' for t in ts)})")
        # the warp launch alone: 20 calls queued behind a busy stream, one event pair
        plans = np.zeros(B, PLAN_DTYPE)
        nbytes = np.array([p.size for p in pages], np.int64)
        plans["src_offset"][1:] = np.cumsum(nbytes[:-1])
        plans["src_h"], plans["src_w"] = [s[0] for s in sizes], [s[1] for s in sizes]
        plans["src_c"] = [1 if p.ndim == 2 else 3 for p in pages]
        dev = torch.device("cuda:0")
        src = torch.from_numpy(np.concatenate([p.reshape(-1) for p in pages])).to(dev)
        dst = torch.empty_like(src)
        d_plans = torch.from_numpy(plans.view(np.uint8).copy()).to(dev)
        d_prm = torch.from_numpy(aug.params(sizes, ids, 0).view(np.uint8).copy()).to(dev)
        assert d_prm.numel() == B * PARAMS_DTYPE.itemsize
        max_side, max_bytes = int(max(max(s) for s in sizes)), int(nbytes.max())

        def launch():
            _lib.check(_lib.lib().i2l_affine_nearest_u8(src.data_ptr(), dst.data_ptr(), d_plans.data_ptr(), d_prm.data_ptr(), B,
                                                        max_side, max_bytes, _lib.stream_ptr()), "affine_nearest_u8")
        busy = torch.randn(4096, 4096, device=dev)
        launch()
        torch.cuda.synchronize()
        per_call = []
        for _ in range(5):
            for _ in range(6):
                busy @ busy                                          # keeps the stream busy while the calls queue up
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                launch()
            e1.record()
            torch.cuda.synchronize()
            per_call.append(e0.elapsed_time(e1) / 20 * 1e3)
        med = statistics.median(per_call)
        lines.append(f"i2l_affine_nearest_u8 alone, HIP events over 20 queued calls: median {med:.1f} us per batch = "
                     f"{2 * src.numel() / med / 1e6:.2f} TB/s read + written (runs: {', '.join(f'{t:.1f}' for t in per_call)})")
    else:
        lines.append("device figures (preprocess_batch with / without augment, the warp launch alone): NOT MEASURED in this "
                     "run (--host-only); the times above are CPU-only timings")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
