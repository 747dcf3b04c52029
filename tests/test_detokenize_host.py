"""The vocabulary image i2l_detokenize reads (training.predictor.token_image), on the host: slot v is
``id_to_token.get(v, UNK)`` in UTF-8, exactly what ``TokenTable.decode`` (tokenizer.py:166-192) looks up per id."""
import os

import numpy as np
import torch

from helpers import GOLDEN
from img2latex_amd.training import TokenTable, token_image
from img2latex_amd.training.predictor import DEFAULT_SPECIAL_TOKENS

SPECIAL = {"<PAD>": 0, "<START>": 1, "<END>": 2, "<UNK>": 3}


def slots(image):
    tok_bytes, tok_off = image[0], image[1]
    assert tok_bytes.dtype == np.uint8 and tok_off.dtype == np.int32 and tok_off[0] == 0 and tok_off[-1] == tok_bytes.size
    assert bool((np.diff(tok_off) >= 0).all())
    raw = tok_bytes.tobytes()
    return [raw[a:b] for a, b in zip(tok_off[:-1], tok_off[1:])]


def test_round_trip_of_slots_and_offsets():
    vocab = dict(SPECIAL)
    vocab.update({f"\\tok{i}": i for i in range(4, 40)})
    tok = TokenTable(vocab)
    image = token_image(tok)
    got = slots(image)
    assert len(got) == 40 and image[2] == [0, 1, 2, 3] and image[3] == 3
    assert {v: s.decode("utf-8") for v, s in enumerate(got)} == tok.id_to_token
    # decode's own lookup, id by id (special ids included: the drop list, not the table, removes them)
    for v in range(40):
        assert got[v].decode("utf-8") == tok.decode([v], skip_special_tokens=False)


def test_gap_in_the_ids_is_the_unk_string():
    vocab = dict(SPECIAL)
    vocab.update({"a": 4, "b": 7, "c": 9})                           # 5, 6, 8 are in no map
    tok = TokenTable(vocab)
    got = slots(token_image(tok))
    assert len(got) == 10
    for v in (5, 6, 8):
        assert got[v] == b"<UNK>" == tok.decode([v], skip_special_tokens=False).encode()
    assert [got[4], got[7], got[9]] == [b"a", b"b", b"c"]


def test_multibyte_utf8_and_the_empty_token():
    vocab = dict(SPECIAL)
    vocab.update({"α": 4, "": 5, "∑x": 6, "𝔽": 7, "\\frac": 8})
    tok = TokenTable(vocab)
    image = token_image(tok)
    got = slots(image)
    assert [len(s) for s in got[4:]] == [2, 0, 4, 4, 5]
    assert image[1][6] - image[1][5] == 0                            # the empty token: an empty slot, offsets still ascend
    ids = [4, 5, 5, 6, 1, 7, 8, 5]
    want = tok.decode(ids)
    assert want == "α   ∑x 𝔽 \\frac "                                # a zero-length token still takes its separators
    assert b" ".join(got[i] for i in ids if i not in image[2]).decode("utf-8") == want


def test_reference_tokenizer_shaped_config():
    """The tokenizer_config the reference's trainer wrote into tests/golden/ref_checkpoint.pt, held by an object that is NOT
    a TokenTable: only id_to_token / token_to_id / special_tokens are read (the attributes of LaTeXTokenizer)."""
    tcfg = torch.load(os.path.join(GOLDEN, "ref_checkpoint.pt"), map_location="cpu", weights_only=False)["tokenizer_config"]

    class LaTeXTokenizerLike:
        def __init__(self):
            self.token_to_id = dict(tcfg["token_to_id"])
            self.id_to_token = {i: t for t, i in self.token_to_id.items()}
            self.special_tokens = dict(tcfg["special_tokens"])

    image = token_image(LaTeXTokenizerLike())
    got = slots(image)
    ref = TokenTable(tcfg["token_to_id"], tcfg["special_tokens"], tcfg["max_sequence_length"])
    assert len(got) == max(ref.id_to_token) + 1
    assert all(got[v].decode("utf-8") == ref.id_to_token[v] for v in ref.id_to_token)
    assert image[2] == sorted(ref.token_to_id[t] for t in ref.special_tokens.values()) and image[3] == ref.unk_token_id


def test_tokenizers_that_keep_the_host_decode():
    class IdOnly:                                                    # the shape of make_golden.py's IdTokenizer
        pad_token_id, start_token_id, end_token_id = 0, 1, 2

        def decode(self, ids):
            return " ".join(map(str, ids))

    assert token_image(IdOnly()) is None
    many = {f"<S{i}>": i for i in range(9)}
    many.update({"<PAD>": 9, "<START>": 10, "<END>": 11, "<UNK>": 12, "x": 13})
    special = dict(DEFAULT_SPECIAL_TOKENS, **{f"S{i}": f"<S{i}>" for i in range(9)})
    assert token_image(TokenTable(many, special)) is None            # 13 special ids: beyond the kernel's 8
    assert token_image(TokenTable(dict(SPECIAL, x=4))) is not None
