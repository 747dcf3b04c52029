"""What the strings cost: Predictor.predict_strings_stream (i2l_detokenize behind every decode, packed bytes + offsets copied
beside the ids, the host only slices) against predict_ids_stream followed by the host TokenTable.decode (the route before
the device detokenizer), in ONE process, alternating; and the HIP-event time of the detokenize launches alone.

B = 256, 150 steps, primary dims, the END-clock weights (rows end between steps ~60 and 150), a 512-token vocabulary of
2 - 15 byte tokens.  usage: python profiles/detokenize_cost.py [--batches N] [--rounds R] [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "hmer-img2latex_amd"))
from img2latex_amd import _lib, synth                                                # noqa: E402
from img2latex_amd.model import Seq2SeqModel                                     # noqa: E402
from img2latex_amd.training import Predictor, TokenTable, detokenize_table       # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "detokenize_cost.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X: a CPU run says nothing about these times"
    dev = torch.device("cuda:0")
    B, T = 256, 150
    cfg = synth.model_config()
    sd_kw = dict(seed=42, out_scale=12.0, enc_scale=16.0, end_clock=(0.05, 12.0, 6.0))
    model = Seq2SeqModel("cnn_lstm", cfg["vocab_size"], synth.encoder_params(cfg), synth.decoder_params(cfg))
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(cfg, **sd_kw).items()})
    model = model.to(dev).eval()
    vocab = {"<PAD>": 0, "<START>": 1, "<END>": 2, "<UNK>": 3}
    vocab.update({f"\\{i:x}" + "x" * ((i * 7) % 12): i for i in range(4, cfg["vocab_size"])})     # 2 - 15 bytes
    tok = TokenTable(vocab, max_sequence_length=T)
    pred = Predictor(model, tok, device=dev)
    x = torch.from_numpy(synth.make_images(B, cfg, seed=1234)).to(dev)

    def strings_route(n):
        out = None
        for out in pred.predict_strings_stream((x for _ in range(n)), max_length=T):
            pass
        return out

    def ids_route(n):
        out = None
        for out in pred.predict_ids_stream((x for _ in range(n)), max_length=T):
            pass
        return out

    def host_route(n):
        out = None
        for seqs in pred.predict_ids_stream((x for _ in range(n)), max_length=T):
            out = [tok.decode(seq[1:]) for seq in seqs]
        return out

    routes = {"predict_strings_stream (device detokenize)": strings_route,
              "predict_ids_stream + host decode (the route before)": host_route,
              "predict_ids_stream alone (ids as lists, no strings)": ids_route}
    a, b = strings_route(12), host_route(12)                         # warm-up of every kernel and pinned buffer
    ids_route(12)
    assert a == b, "the two routes disagree"
    lens = [len(s.split(" ")) if s else 0 for s in a]
    times = {k: [] for k in routes}
    for _ in range(args.rounds):
        for name, fn in routes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(args.batches)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / args.batches * 1e3)

    # the detokenize launches alone, on the ids of one decode: 20 calls queued behind a busy stream, one event pair
    table = detokenize_table(tok, dev)
    with torch.no_grad():
        ids, _ = model.greedy_ids(model.encoder(x), synth.START, synth.END, T, stop=_lib.STOP_STICKY, select=_lib.SELECT_SOFTMAX)
    side = torch.cuda.Stream(device=dev)
    bufs = table.buffers(B, T)
    busy = torch.randn(4096, 4096, device=dev)
    torch.cuda.synchronize()
    per_call, host_call = [], []
    with torch.cuda.stream(side):
        table.launch(ids, synth.END, bufs)
        for _ in range(5):
            for _ in range(6):
                busy @ busy                                          # keeps the stream busy while the calls queue up
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(side)
            t0 = time.perf_counter()
            for _ in range(20):
                table.launch(ids, synth.END, bufs)
            host_call.append((time.perf_counter() - t0) / 20 * 1e6)
            e1.record(side)
            side.synchronize()
            per_call.append(e0.elapsed_time(e1) / 20 * 1e3)
    total_bytes = int(bufs[1][B].item())

    lines = [f"detokenize_cost: B={B}, steps={T}, vocab={cfg['vocab_size']}, tokens kept per row min/mean/max = "
             f"{min(lens)}/{sum(lens) / len(lens):.1f}/{max(lens)}, {total_bytes} bytes of text per batch, "
             f"{args.batches} batches per timing, {args.rounds} rounds (alternating)", ""]
    for name, ts in times.items():
        lines.append(f"{name}: median {statistics.median(ts):.3f} ms per batch (rounds: {', '.join(f'{t:.3f}' for t in ts)})")
    lines.append(f"i2l_detokenize, 3 launches, HIP events over 20 queued calls: median {statistics.median(per_call):.1f} us per call "
                 f"(runs: {', '.join(f'{t:.1f}' for t in per_call)}); host time of the call itself "
                 f"{statistics.median(host_call):.1f} us (it reads the offset table back before launching)")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
