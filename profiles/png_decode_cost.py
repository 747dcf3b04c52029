"""What building the page store costs with the page files decoded on the host (PIL) and on the device (i2l_png_decode).

Synthetic stroke pages -- white, with dark pen strokes -- of bench.py's `--mode preprocess` shapes (30 - 119 x 80 - 779
pixels, L and RGB alternating), saved as PNG by PIL (its default compression and per-row filter choice) into a temporary
directory; 256 and 4096 of them.

    host      PageStore(decode="host"):   decode (PIL, `--decode-threads` threads) and upload (pinned chunks), split as in
              profiles/dataset_cost.txt
    device    PageStore(decode="device"): read + parse (the same threads: file read, chunk walk, CRCs), upload (packing
              and copying the compressed streams), launch (i2l_png_decode until its status words are back) and fallback
              (PIL + pinned upload of the files the device did not take; none here)

Each route is built `--builds` times, alternating; the first build of each also pays first-use set-up and is listed but
left out of the median.  `wall` is the whole constructor.  The two stores are compared page by page first.
Needs the MI355X: without a device it fails.
usage: python profiles/png_decode_cost.py [--builds N] [--decode-threads T] [--sizes 256,4096] [--out FILE]"""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "hmer-img2latex_amd"))


def stroke_page(k):
    h, w, c = 30 + (7 * k) % 90, 80 + (53 * k) % 700, 1 + 2 * (k % 2)
    rng = np.random.default_rng(9000 + k)
    page = np.full((h, w), 255, np.uint8)
    for _ in range(max(4, w // 12)):                                  # short strokes, two or three pixels thick
        y, x = int(rng.integers(0, h)), int(rng.integers(0, w))
        dy, dx = rng.integers(-1, 2), rng.integers(-1, 2)
        ink = int(rng.integers(0, 120))
        for s in range(int(rng.integers(4, 24))):
            yy, xx = y + s * dy, x + s * dx
            if 0 <= yy < h and 0 <= xx < w:
                page[max(0, yy - 1):yy + 1, max(0, xx - 1):xx + 2] = ink
    return page if c == 1 else np.stack([page, page, np.minimum(page, 250)], axis=2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--builds", type=int, default=4)
    ap.add_argument("--decode-threads", type=int, default=8)
    ap.add_argument("--sizes", default="256,4096")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png_decode_cost.txt"))
    args = ap.parse_args()
    import torch
    from PIL import Image
    from img2latex_amd.data import PageStore
    assert torch.cuda.is_available(), "png_decode_cost measures the device path: it needs the MI355X"
    dev = torch.device("cuda:0")
    torch.zeros(1, device=dev)                                       # the context is not part of any figure
    lines = []
    for n in [int(v) for v in args.sizes.split(",")]:
        with tempfile.TemporaryDirectory() as root:
            paths, decoded = [], 0
            for k in range(n):
                page = stroke_page(k)
                decoded += page.size
                paths.append(os.path.join(root, f"{k:05d}.png"))
                Image.fromarray(page).save(paths[-1])
            on_disk = sum(os.path.getsize(p) for p in paths)
            lines.append(f"png_decode_cost: {n} stroke pages, {decoded / 1e6:.1f} MB decoded, {on_disk / 1e6:.2f} MB of PNG files, "
                         f"{args.decode_threads} host threads, {args.builds} builds per route")
            host = PageStore(paths, 3, dev, args.decode_threads)
            device = PageStore(paths, 3, dev, args.decode_threads, decode="device")
            assert not host.failed.any() and not device.failed.any() and np.array_equal(host.shapes, device.shapes)
            for r in range(n):
                size = int(np.prod(host.shapes[r]))
                assert torch.equal(host.pixels[host.offsets[r]:host.offsets[r] + size],
                                   device.pixels[device.offsets[r]:device.offsets[r] + size]), r
            rows = {"host": [], "device": []}
            for _ in range(args.builds):
                for route in ("host", "device"):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    store = PageStore(paths, 3, dev, args.decode_threads, decode=route)
                    torch.cuda.synchronize()
                    wall = time.perf_counter() - t0
                    if route == "host":
                        rows[route].append((wall, store.decode_seconds, store.upload_seconds))
                    else:
                        s = store.seconds
                        rows[route].append((wall, s["read_parse"], s["upload"], s["launch"], s["fallback"]))
                    del store
            names = {"host": ("wall", "decode (PIL)", "upload (pinned chunks)"),
                     "device": ("wall", "read + parse", "upload (compressed)", "launch (i2l_png_decode)", "fallback")}
            for route in ("host", "device"):
                for col, name in enumerate(names[route]):
                    vals = [row[col] * 1e3 for row in rows[route]]
                    med = statistics.median(vals[1:]) if len(vals) > 1 else vals[0]
                    rate = f" = {n / med:.1f} k pages/s" if col == 0 else ""
                    lines.append(f"  {route}, {name}: median {med:.2f} ms{rate} (builds: {', '.join(f'{v:.2f}' for v in vals)}; "
                                 "the first is left out of the median)")
            lines.append("")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
