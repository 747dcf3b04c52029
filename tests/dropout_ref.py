"""The training decoder's dropout masks, restated ("The dropout mask rule"): plain numpy and torch,
nothing imported from the library.  The kernels never store a mask; forward and backward both recompute it from
(seed, stream, element index), so the rule can be evaluated here, bit for bit, and the whole masked forward written down
as a differentiable function of float64 inputs (decoder_forward_masked follows oracle/img2latex_oracle.py's
decoder_forward and lstm_step, each F.dropout replaced by a multiplication with the restated mask).

tests/test_train_dropout_gpu.py pins this restatement to the kernels element for element; the statistics of
tests/test_train_dropout_host.py mean something only because of that."""
import numpy as np
import torch
import torch.nn.functional as F

DS_X, DS_OUT, DS_LAYER0 = 1, 2, 8           # streams: LSTM input, LSTM output, inter-layer l = DS_LAYER0 + l
_M64 = (1 << 64) - 1
_GOLDEN, _STREAM = 0x9E3779B97F4A7C15, 0xD1B54A32D192ED03
_MUL1, _MUL2 = 0xBF58476D1CE4E5B9, 0x94D049BB133111EB


def uniforms(seed, stream, n, start=0):
    """float32 u in [0, 1) of the elements start .. start + n - 1: uint64 arithmetic that wraps."""
    idx = np.arange(start, start + n, dtype=np.uint64)
    base = np.uint64(((int(seed) & _M64) + int(stream) * _STREAM) & _M64)
    z = idx * np.uint64(_GOLDEN) + base                           # arrays of uint64 wrap silently
    z = (z ^ (z >> np.uint64(30))) * np.uint64(_MUL1)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(_MUL2)
    z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)      # 24 bits: exact in float32


def keep_mask(seed, stream, n, p):
    """bool (n,): element idx is kept iff u(seed, stream, idx) >= float32(p).  p <= 0 keeps everything."""
    if not p > 0:
        return np.ones(n, dtype=bool)
    return uniforms(seed, stream, n) >= np.float32(p)


def scale(p):
    """The factor of a kept element: 1 / (1 - p) evaluated in float32 as the kernels do, then widened."""
    if not p > 0:
        return 1.0
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def mask_tensor(seed, stream, shape, p, like):
    """keep_mask * scale of ``shape`` (row-major element index) in the dtype and on the device of ``like``."""
    n = int(np.prod(shape))
    m = torch.from_numpy(keep_mask(seed, stream, n, p)).to(like.device).to(like.dtype) * scale(p)
    return m.view(*shape)


def _attention_context(sd, h_top, enc):
    """oracle attention_context: over a source of length 1 the context equals enc and the parameters get exact zeros."""
    hid = h_top.repeat(1, enc.shape[1], 1)
    energy = torch.tanh(F.linear(torch.cat((hid, enc), dim=2), sd["decoder.attention.attn.weight"],
                                 sd["decoder.attention.attn.bias"]))
    score = F.linear(energy, sd["decoder.attention.v.weight"]).squeeze(2)
    return torch.bmm(F.softmax(score, dim=1).unsqueeze(1), enc)


def decoder_forward_masked(sd, cfg, enc, tokens, p, seed, tape=None):
    """LSTMDecoder.forward in training mode with the kernels' masks -> logits (B, T, V), in enc's dtype, differentiable
    in enc and every tensor of ``sd`` ("decoder." keys).  With bt = b T + t:
      X, plain path       the whole (B T, 2E) row           flat index bt 2E + e
      X, attention path   the embedding half only           bt E + e
      inter-layer l       the output of layer l < L - 1     bt H + j     stream DS_LAYER0 + l
      OUT                 the top layer's h                 bt H + j
    ``tape``: a dict that receives, per step t, the intermediate tensors a test needs to know what a mask multiplied
    (each keeps its gradient after a backward): "x"[t] the LSTM input after its mask (B, 2E); "h"[l][t] the raw output
    of layer l; "below"[l][t] what layer l hands on after its mask (the input of layer l + 1; l < L - 1);
    "cell"[l][t] = (i, g, o, c), detached."""
    B, T = tokens.shape
    E, H, L = cfg["embedding_dim"], cfg["hidden_dim"], cfg["lstm_layers"]
    emb = F.embedding(tokens.long(), sd["decoder.embedding.weight"])                  # (B, T, E)
    if cfg["attention"]:
        emb = emb * mask_tensor(seed, DS_X, (B, T, E), p, enc)                        # decoder.py:162
    else:
        m_x = mask_tensor(seed, DS_X, (B, T, 2 * E), p, enc)                          # decoder.py:130-133
    m_layer = [mask_tensor(seed, DS_LAYER0 + l, (B, T, H), p, enc) for l in range(L - 1)]
    m_out = mask_tensor(seed, DS_OUT, (B, T, H), p, enc)
    h = [torch.zeros(B, H, dtype=enc.dtype, device=enc.device) for _ in range(L)]
    c = [torch.zeros(B, H, dtype=enc.dtype, device=enc.device) for _ in range(L)]
    outs = []
    if tape is not None:
        tape.update(x=[], h=[[] for _ in range(L)], below=[[] for _ in range(L)], cell=[[] for _ in range(L)])

    def keep(where, v):
        if tape is not None:
            if v.requires_grad:
                v.retain_grad()
            where.append(v)
        return v

    for t in range(T):
        if cfg["attention"]:
            ctx = _attention_context(sd, h[-1].unsqueeze(1), enc.unsqueeze(1)).squeeze(1)
            inp = torch.cat([emb[:, t, :], ctx], dim=1)
        else:
            inp = torch.cat([emb[:, t, :], enc], dim=1) * m_x[:, t, :]
        if tape is not None:
            inp = keep(tape["x"], inp)
        for l in range(L):
            gates = (F.linear(inp, sd[f"decoder.lstm.weight_ih_l{l}"], sd[f"decoder.lstm.bias_ih_l{l}"])
                     + F.linear(h[l], sd[f"decoder.lstm.weight_hh_l{l}"], sd[f"decoder.lstm.bias_hh_l{l}"]))
            i, f, g, o = gates.split(H, dim=1)
            c[l] = torch.sigmoid(f) * c[l] + torch.sigmoid(i) * torch.tanh(g)
            h[l] = torch.sigmoid(o) * torch.tanh(c[l])
            if tape is not None:
                h[l] = keep(tape["h"][l], h[l])
                tape["cell"][l].append(tuple(v.detach() for v in (torch.sigmoid(i), torch.tanh(g), torch.sigmoid(o), c[l])))
            inp = h[l] * m_layer[l][:, t, :] if l < L - 1 else h[l]                   # decoder.py:81
            if tape is not None and l < L - 1:
                inp = keep(tape["below"][l], inp)
        outs.append(F.linear(inp * m_out[:, t, :], sd["decoder.output_layer.weight"],
                             sd["decoder.output_layer.bias"]))                        # decoder.py:139 / :186
    return torch.stack(outs, dim=1)
