"""What a batch costs from the device-resident data set, against the path it replaces, and what building the stores costs.

256 pages of bench.py's `--mode preprocess` shapes (30 - 119 x 80 - 779 pixels, L and RGB alternating, written as PNG
into a temporary data directory) with formulas of 40 - 147 tokens -> (256, 3, 64, 320) images + the padded id matrix.

    resident    DeviceDataset(resident=True).batch(indices): one small upload (indices, plans, table requests, gather
                list), i2l_collate_ids + i2l_gather_ragged_u8 + the preprocessing chain
    streaming   what the parent commit did per batch with the pages already decoded: preprocess_batch from the host
                arrays (pack + upload of the pixels) + TokenizeTable.collate from the strings
    build       one-time: decode (PIL, `--decode-threads` threads), upload (chunks through pinned memory), tokenize
                (corpus upload + i2l_tokenize_packed + the offsets' copy back)

Per route: `host` = wall time of the call alone (the enqueue; nothing waits for the device except what the route itself
waits for), `period` = wall time per batch of N back-to-back calls ending in a device synchronise.  The routes alternate
inside every round; medians over the rounds.  Needs the MI355X: without a device it fails.
usage: python profiles/dataset_cost.py [--batches N] [--rounds R] [--decode-threads T] [--out FILE]"""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "hmer-img2latex_amd"))
from img2latex_amd import synth                                                  # noqa: E402


def make_pages(n):
    sizes = [(30 + (7 * k) % 90, 80 + (53 * k) % 700, 1 + 2 * (k % 2)) for k in range(n)]
    return [np.round(synth.uniform(5000 + k, "img", (h, w, c), 0.0, 255.0)).astype(np.uint8).reshape((h, w) if c == 1 else (h, w, 3))
            for k, (h, w, c) in enumerate(sizes)]


def write_data_dir(root, pages, vocab):
    from PIL import Image
    os.makedirs(os.path.join(root, "img"))
    lines, split = [], []
    for k, p in enumerate(pages):
        Image.fromarray(p).save(os.path.join(root, "img", f"{k:04d}.png"))
        n_tok = 40 + (37 * k) % 108                                  # 40 .. 147
        lines.append(" ".join(vocab[(11 * k + 7 * j) % len(vocab)] for j in range(n_tok)))
        split.append(f"{k:04d}.png {k}")
    with open(os.path.join(root, "formulas.lst"), "w") as f:
        f.write("\n".join(lines) + "\n")
    with open(os.path.join(root, "split.lst"), "w") as f:
        f.write("\n".join(split) + "\n")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--decode-threads", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dataset_cost.txt"))
    args = ap.parse_args()
    import torch
    from img2latex_amd.data import DeviceDataset, preprocess_batch
    from img2latex_amd.training import TokenTable, tokenize_table
    assert torch.cuda.is_available(), "dataset_cost measures the device path: it needs the MI355X"
    dev = torch.device("cuda:0")
    B = 256
    pages = make_pages(B)
    words = [f"\\tok{i}" for i in range(496)]
    tok = TokenTable({**{"<PAD>": 0, "<START>": 1, "<END>": 2, "<UNK>": 3}, **{w: 4 + i for i, w in enumerate(words)}},
                     max_sequence_length=150)
    lines = [f"dataset_cost: {B} pages, {sum(p.size for p in pages) / 1e6:.1f} MB decoded, formulas of 40 - 147 tokens, "
             f"{args.batches} batches x {args.rounds} rounds, -> ({B}, 3, 64, 320)", ""]
    with tempfile.TemporaryDirectory() as root:
        formulas = write_data_dir(root, pages, words)
        torch.zeros(1, device=dev)                                   # the context is not part of any figure
        preprocess_batch(pages[:4], (64, 320), 3, True, device=dev)
        builds = []
        for r in range(3):                                           # the first build also loads the kernels: reported apart
            ds = DeviceDataset(root, "split.lst", "formulas.lst", tok, img_size=(64, 320), channels=3, resident=True,
                               device=dev, decode_threads=args.decode_threads)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ds.formulas.build()
            torch.cuda.synchronize()
            t_tok = time.perf_counter() - t0
            ds.build()
            torch.cuda.synchronize()
            builds.append((ds.pages.decode_seconds * 1e3, ds.pages.upload_seconds * 1e3, t_tok * 1e3))
        for name, col in (("decode (PIL, %d threads)" % args.decode_threads, 0), ("upload (pinned chunks)", 1),
                          ("tokenize (corpus upload + i2l_tokenize_packed + offsets back)", 2)):
            vals = [b[col] for b in builds]
            lines.append(f"build, {name}: median {statistics.median(vals):.2f} ms for {B} pages / formulas "
                         f"(builds: {', '.join(f'{v:.2f}' for v in vals)}; the first one includes first-use set-up)")
        lines.append(f"store: {ds.pages.pixels.numel() / 1e6:.1f} MB of pages, {ds.formulas.n_ids} ids")
        lines.append("")
        table = tokenize_table(tok, dev)
        rng = np.random.default_rng(0)
        perms = [rng.permutation(B) for _ in range(args.batches)]

        def resident(idx):
            return ds.batch(idx)

        def streaming(idx):
            return preprocess_batch([pages[i] for i in idx], (64, 320), 3, True, device=dev), \
                table.collate([formulas[i] for i in idx])

        routes = {"resident": resident, "streaming": streaming}
        # same results first (images bit for bit, ids equal), which is also the warm-up of every shape
        for idx in perms[:10]:
            a, (x, ids) = resident(idx), streaming(idx)
            assert torch.equal(a["images"], x) and torch.equal(a["formulas"], ids)
        host = {k: [] for k in routes}
        period = {k: [] for k in routes}
        for _ in range(args.rounds):
            for name, fn in routes.items():
                torch.cuda.synchronize()
                calls = 0.0
                t0 = time.perf_counter()
                for idx in perms:
                    c0 = time.perf_counter()
                    fn(idx)
                    calls += time.perf_counter() - c0
                torch.cuda.synchronize()
                period[name].append((time.perf_counter() - t0) / len(perms) * 1e3)
                host[name].append(calls / len(perms) * 1e3)
        for name in routes:
            lines.append(f"{name}: host {statistics.median(host[name]):.3f} ms per batch, period "
                         f"{statistics.median(period[name]):.3f} ms per batch = "
                         f"{B / statistics.median(period[name]):.0f} k images/s (rounds, host: "
                         f"{', '.join(f'{t:.3f}' for t in host[name])}; period: {', '.join(f'{t:.3f}' for t in period[name])})")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
