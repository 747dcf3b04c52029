"""The embedding gradient of the decoder's backward pass (csrc/train_decoder.hip, emb_gather_kernel) on its own:
dEmb[v] = sum over the positions bt with tok[bt] == v of dX[bt][:E] * mask, summed in a FIXED order.

i2l_decoder_train_bwd reads its token array for this sum only, so the same forward pass and the same dlogits can be
pushed through two backward calls: one with the real tokens, one with the tokens replaced by 0, 1, 2, ... (V >= B*T),
whose row bt of dEmb is then the contribution of position bt alone.  From those contributions the test states the sum
twice: in float64, with the bound of a recursive fp32 sum of n terms, (n - 1) * 2^-24 * sum |terms|; and in fp32 in the
kernel's documented order (tokens scanned 256 at a time, a chunk's hits of one id dealt to four partial sums in turn,
the four added in order), which the result must equal bit for bit.  With the dropout probabilities used (0 and 0.5) the
mask scale is 1 or 2, so a contribution is the same number whether or not the kernel fuses scale and add."""
import numpy as np
import pytest
import torch

from conftest import record
from img2latex_amd import synth
from img2latex_amd.model import Seq2SeqModel
from img2latex_amd.model._train_fn import decoder_train_backward, decoder_train_forward

pytestmark = pytest.mark.gpu
DEV = "cuda"
V = 1100

#        E    B   T   attention  dropout     E on both sides of the 64-column groups, B*T on both sides of the 256 chunk
CASES = [(4, 5, 12, False, 0.0),
         (36, 37, 7, True, 0.5),          # 259 positions: one full chunk and a tail of 3
         (64, 16, 16, False, 0.5),        # exactly one chunk, exactly one column group
         (100, 64, 16, True, 0.0),        # 1024 = four chunks, two column groups with a tail of 36
         (192, 257, 4, False, 0.0),       # 1028: four chunks and a tail of 4; three full column groups
         (68, 64, 17, False, 0.5)]        # 1088; a second column group of 4


def _decoder(E, attention, dropout):
    cfg = synth.model_config(vocab_size=V, embedding_dim=E, hidden_dim=64, lstm_layers=1, attention=attention,
                             channels=1, img_height=16, img_width=32, conv_filters=(4, 8, 16))
    sd = synth.make_state_dict(cfg, seed=300 + E, out_scale=8.0)
    m = Seq2SeqModel("cnn_lstm", V, synth.encoder_params(cfg), synth.decoder_params(cfg))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    dec = m.to(DEV).decoder
    dec.train()
    dec.dropout = dropout
    return dec


def _tokens(B, T, rng):
    """A few ids, so that one id has many hits inside a chunk and across chunks: a run of one id over 300 positions
    (where there are that many), ids below 0 and above V - 1 (clamped to rows 0 and V - 1), the rest from six ids."""
    ids = np.asarray([0, 1, 7, 513, V - 2, V - 1, -3, V + 5], dtype=np.int32)
    tok = ids[rng.integers(0, len(ids), size=B * T)]
    if B * T > 400:
        tok[200:500] = 7
    return tok.reshape(B, T)


def _kernel_order_sum(tok, contrib):
    """fp32, in the order the kernel documents: per id, hit h (counted within its chunk of 256 positions) goes to
    partial sum h % 4; dEmb[v] = ((s0 + s1) + s2) + s3."""
    BT, E = contrib.shape
    part = np.zeros((V, 4, E), dtype=np.float32)
    for c0 in range(0, BT, 256):
        seen = {}
        for bt in range(c0, min(c0 + 256, BT)):
            v = int(tok[bt])
            h = seen.get(v, 0)
            seen[v] = h + 1
            part[v, h % 4] += contrib[bt]
    return ((part[:, 0] + part[:, 1]) + part[:, 2]) + part[:, 3]


@pytest.mark.parametrize("E,B,T,attention,dropout", CASES)
def test_embedding_gradient_is_the_fixed_order_sum(E, B, T, attention, dropout):
    rng = np.random.default_rng(E * 1000 + B)
    dec = _decoder(E, attention, dropout)
    BT = B * T
    assert BT <= V
    tok = _tokens(B, T, rng)
    tokens = torch.from_numpy(tok).to(DEV)
    alone = torch.arange(BT, dtype=torch.int32, device=DEV).reshape(B, T)
    enc = torch.from_numpy(rng.uniform(-1.5, 1.5, size=(B, E)).astype(np.float32)).to(DEV)
    dlogits = torch.from_numpy(rng.standard_normal((B, T, V)).astype(np.float32)).to(DEV)

    def backward(tokens_for_the_gradient):
        _, state = decoder_train_forward(dec, enc, tokens, seed=11)
        state["tokens"] = tokens_for_the_gradient
        grads = {n: torch.full_like(p, float("nan")) for n, p in dec.named_parameters()}
        denc = decoder_train_backward(dec, state, dlogits, grads)
        torch.cuda.synchronize()
        return {n: g.cpu() for n, g in grads.items()}, denc.cpu()

    first, denc1 = backward(tokens)
    again, denc2 = backward(tokens)
    single, denc3 = backward(alone)
    for n in first:                                          # two launches: the same bits, every gradient
        assert torch.equal(first[n], again[n]), n
        if n != "embedding.weight":                          # and the token array reaches the embedding gradient only
            assert torch.equal(first[n], single[n]), n
    assert torch.equal(denc1, denc2) and torch.equal(denc1, denc3)
    got = first["embedding.weight"].numpy()
    contrib = single["embedding.weight"].numpy()
    assert np.isfinite(got).all() and np.isfinite(contrib).all()          # every element was written
    assert not contrib[BT:].any() and np.abs(contrib[:BT]).max() > 0
    if dropout > 0:                                          # the mask drops about half of the embedding columns
        assert 0.3 < float((contrib[:BT] == 0).mean()) < 0.7
    contrib = contrib[:BT]
    clamped = np.clip(tok.reshape(-1), 0, V - 1)
    want64 = np.zeros((V, E))
    mag = np.zeros((V, E))
    np.add.at(want64, clamped, contrib.astype(np.float64))
    np.add.at(mag, clamped, np.abs(contrib).astype(np.float64))
    hits = np.bincount(clamped, minlength=V)
    assert hits.max() >= (300 if BT > 400 else 2)
    assert not got[hits == 0].any()                          # rows without a hit are exactly zero
    bound = np.maximum(hits - 1, 0)[:, None] * 2.0 ** -24 * mag
    err = np.abs(got - want64)
    record("embedding gradient vs float64 [err / ((n - 1) 2^-24 sum|terms|), worst row]",
           float((err / (bound + 1e-300))[hits > 1].max()))
    assert (err <= bound).all(), (E, B, T)
    assert np.array_equal(got, _kernel_order_sum(clamped, contrib)), (E, B, T)
