"""Train-time augmentation on the device (csrc/augment.hip) against Pillow's recorded bytes (tests/golden/
augment_pillow.npz) and the numpy restatement (tests/augment_ref.py).  A gather: every comparison is exact."""
import numpy as np
import pytest
import torch
import yaml

import augment_ref as R
from helpers import GOLDEN
from img2latex_amd import _lib
from img2latex_amd.data import Augment, preprocess_batch
from img2latex_amd.data import augment as A
from img2latex_amd.data.preprocess import PLAN_DTYPE

pytestmark = pytest.mark.gpu
DEV = "cuda"


class FixedAugment(Augment):
    """The given (angle, tx, ty) per page in place of the random draw."""

    def __init__(self, angles, tx, ty):
        super().__init__()
        self.fixed = (np.asarray(angles, np.float64), np.asarray(tx, np.int64), np.asarray(ty, np.int64))

    def draw(self, sizes, sample_ids, epoch=0):
        return self.fixed


@pytest.fixture(scope="module")
def fixture():
    """Pages, parameters and Pillow's outputs of every fixture case, computed once and left unchanged."""
    d = np.load(f"{GOLDEN}/augment_pillow.npz")
    seen, pages, params, outs = {}, [], [], []
    for (c, si, a, tx, ty) in R.fixture_cases():
        h, w = R.SIZES[si]
        j = seen.get((c, si), 0)
        seen[(c, si)] = j + 1
        pages.append(R.fixture_page(c, si))
        params.append(R.coefficients(a, w, h) + (tx, ty))
        outs.append(d[f"out_c{c}_s{si}"][j])
    return pages, params, outs


def canary(n):
    return ((np.arange(n, dtype=np.int64) * 37 + 11) % 251).astype(np.uint8)


def run_u8(pages, params, gaps):
    """One launch over the ragged batch, `gaps[i]` unused bytes in front of page i and a tail behind the last.  Returns
    (out buffer, offsets) with the out buffer pre-filled with the canary."""
    n = len(pages)
    plans = np.zeros(n, PLAN_DTYPE)
    off = 0
    for i, p in enumerate(pages):
        off += gaps[i]
        plans[i]["src_offset"], plans[i]["src_h"], plans[i]["src_w"] = off, p.shape[0], p.shape[1]
        plans[i]["src_c"] = 1 if p.ndim == 2 else 3
        off += p.size
    total = off + 29
    src = np.full(total, 7, np.uint8)
    for p, pl in zip(pages, plans):
        src[pl["src_offset"]:pl["src_offset"] + p.size] = p.reshape(-1)
    prm = np.zeros(n, A.PARAMS_DTYPE)
    for i, t in enumerate(params):
        prm[i] = t
    d_src = torch.from_numpy(src).to(DEV)
    d_out = torch.from_numpy(canary(total)).to(DEV)
    d_plans = torch.from_numpy(plans.view(np.uint8).copy()).to(DEV)
    d_prm = torch.from_numpy(prm.view(np.uint8).copy()).to(DEV)
    rc = _lib.lib().i2l_affine_nearest_u8(d_src.data_ptr(), d_out.data_ptr(), d_plans.data_ptr(), d_prm.data_ptr(), n,
                                          max(max(p.shape[:2]) for p in pages), max(p.size for p in pages), _lib.stream_ptr())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert torch.equal(d_src.cpu(), torch.from_numpy(src))                  # the input is only read
    return d_out.cpu().numpy(), plans["src_offset"].tolist()


def test_u8_ragged_batch_equals_pillow(fixture):
    """All 180 cases -- mixed sizes, mixed src_c, page starts at every residue of the 8-byte store -- in one launch:
    Pillow's bytes on the pages, the canary everywhere else."""
    pages, params, outs = fixture
    gaps = [(5 * i) % 13 for i in range(len(pages))]
    got, offs = run_u8(pages, params, gaps)
    assert {o % 8 for o in offs} == set(range(8))
    want = canary(len(got))
    for o, w in zip(offs, outs):
        want[o:o + w.size] = w.reshape(-1)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad.size, bad[:8].tolist())


def test_u8_packed_batch_and_identity(fixture):
    """Pages back to back (preprocess_batch's layout: no gaps); angle 0 with zero shift returns the input bytes."""
    pages, params, outs = fixture
    sel = list(range(0, len(pages), 7))
    got, offs = run_u8([pages[i] for i in sel], [params[i] for i in sel], [0] * len(sel))
    for i, o in zip(sel, offs):
        assert np.array_equal(got[o:o + pages[i].size], outs[i].reshape(-1)), i
    assert np.array_equal(got[offs[-1] + pages[sel[-1]].size:], canary(len(got))[offs[-1] + pages[sel[-1]].size:])
    ident = [A.coefficients(0.0, p.shape[1], p.shape[0]) + (0, 0) for p in pages[::9]]
    got, offs = run_u8(pages[::9], ident, [3] * len(ident))
    for p, o in zip(pages[::9], offs):
        assert np.array_equal(got[o:o + p.size], p.reshape(-1))


@pytest.mark.parametrize("shape", [(3, 1, 7, 13), (2, 3, 33, 2), (2, 3, 51, 403), (5, 1, 1, 9), (2, 4, 64, 321)])
def test_f32_equals_restatement(shape):
    """Dense fp32 planes, distinct per-channel fills, more than one block per image at the larger shapes, odd widths (a
    16-byte store then starts at every residue): bit-equal to the gather applied to the planes."""
    b, c, h, w = shape
    x = np.stack([np.stack([R.make_page(900 + 10 * i + ch, h, w, 1) for ch in range(c)]) for i in range(b)])
    x = (x.astype(np.float32) / np.float32(255.0) * np.float32(2.0) - np.float32(1.0)).astype(np.float32)
    fill = tuple(np.float32(v) for v in (1.0, 2.2489083, -0.5, 3.25)[:c])
    angles, tx, ty = [5.0, -3.999, 0.0001, 0.0, 1.2345][:b], [3, -6, 0, 0, 1][:b], [-1, 1, 0, 0, 0][:b]
    aug = FixedAugment(angles, tx, ty)
    got = aug.tensor(torch.from_numpy(x).to(DEV), fill)
    torch.cuda.synchronize()
    want = np.stack([R.warp_planes(x[i], R.coefficients(angles[i], w, h), tx[i], ty[i], fill) for i in range(b)])
    assert got.dtype == torch.float32 and tuple(got.shape) == shape
    assert np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32))
    if b > 3:                                                               # image 3: angle 0, zero shift
        assert np.array_equal(got[3].cpu().numpy(), x[3])


def test_tensor_draws_per_sample():
    """Augment.tensor with its own draws: the warp of a sample follows its id, not its place in the batch."""
    aug = Augment(seed=9)
    x = torch.from_numpy(np.stack([R.make_page(40 + i, 16, 48, 1)[None] for i in range(4)]).astype(np.float32)).to(DEV)
    a = aug.tensor(x, (1.0,), [10, 11, 12, 13], epoch=3)
    b = aug.tensor(x.flip(0).contiguous(), (1.0,), [13, 12, 11, 10], epoch=3)
    assert torch.equal(a, b.flip(0)) and not torch.equal(a, x)
    p = aug.params([(16, 48)] * 4, [10, 11, 12, 13], epoch=3)
    want = np.stack([R.warp_planes(x[i].cpu().numpy(), tuple(p[i])[:6], p[i]["tx"], p[i]["ty"], (1.0,)) for i in range(4)])
    assert np.array_equal(a.cpu().numpy(), want)
    with pytest.raises(RuntimeError):
        aug.tensor(x.cpu(), (1.0,))


@pytest.mark.parametrize("channels", [1, 3])
def test_preprocess_batch_with_augment_equals_pillow_pages(fixture, channels):
    """The reference's order on raw pages: preprocess_batch(pages, augment=A) == preprocess_batch(Pillow's warped pages),
    and augment=None == the call without the keyword."""
    pages, params, outs = fixture
    cases = R.fixture_cases()
    sel = list(range(len(pages)))
    aug = FixedAugment([cases[i][2] for i in sel], [cases[i][3] for i in sel], [cases[i][4] for i in sel])
    got = preprocess_batch([pages[i] for i in sel], (64, 320), channels, True, augment=aug)
    want = preprocess_batch([outs[i] for i in sel], (64, 320), channels, True)
    plain = preprocess_batch([pages[i] for i in sel], (64, 320), channels, True)
    none = preprocess_batch([pages[i] for i in sel], (64, 320), channels, True, augment=None)
    assert torch.equal(got, want) and torch.equal(plain, none) and not torch.equal(got, plain)
    # a drawn warp, on the table pool's path and a side upload stream
    drawn = Augment(seed=2)
    ids = np.arange(len(sel)) + 50
    prm = drawn.params([pages[i].shape[:2] for i in sel], ids, 1)
    warped = [R.warp_pages(pages[i], tuple(prm[k])[:6], prm[k]["tx"], prm[k]["ty"]) for k, i in enumerate(sel)]
    side = torch.cuda.Stream()
    got = preprocess_batch([pages[i] for i in sel], (64, 320), channels, True, tables="host", upload_stream=side,
                           augment=drawn, sample_ids=ids, epoch=1)
    assert torch.equal(got, preprocess_batch(warped, (64, 320), channels, True))


def test_preprocess_none_matches_recorded_output():
    """augment=None is today's output: the reference's recorded tensor of the preprocessing fixture."""
    d = np.load(f"{GOLDEN}/preprocess.npz")
    h, w, c, th, tw, oc = d["cases"][0].tolist()
    page = R.make_page(1000, h, w, c)
    got = preprocess_batch([page], (th, tw), oc, True, augment=None)[0]
    assert np.array_equal(got.cpu().numpy(), d["out0"])
    same = preprocess_batch([page], (th, tw), oc, True, augment=Augment(degrees=0.0, translate=(0.0, 0.0)))[0]
    assert np.array_equal(same.cpu().numpy(), d["out0"])


def test_oversized_side_is_refused_without_a_launch():
    L = _lib.lib()
    src = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    out = torch.from_numpy(canary(4096)).to(DEV)
    plans = np.zeros(1, PLAN_DTYPE)
    plans[0]["src_h"], plans[0]["src_w"], plans[0]["src_c"] = 1, 16385, 1    # the launch would write 16385 bytes
    d_plans = torch.from_numpy(plans.view(np.uint8).copy()).to(DEV)
    prm = np.zeros(1, A.PARAMS_DTYPE)
    prm[0] = A.coefficients(0.0, 16385, 1) + (0, 0)
    d_prm = torch.from_numpy(prm.view(np.uint8).copy()).to(DEV)
    rc = L.i2l_affine_nearest_u8(src.data_ptr(), out.data_ptr(), d_plans.data_ptr(), d_prm.data_ptr(), 1, 16385, 16385,
                                 _lib.stream_ptr())
    assert rc == _lib.ERR_UNSUPPORTED
    x = torch.zeros(64, dtype=torch.float32, device=DEV)
    y = torch.full((64,), 3.0, dtype=torch.float32, device=DEV)
    fill = np.ones(1, np.float32)
    assert L.i2l_affine_nearest_f32(x.data_ptr(), y.data_ptr(), d_prm.data_ptr(), fill.ctypes.data, 1, 1, 1, 16385,
                                    _lib.stream_ptr()) == _lib.ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), canary(4096)) and bool((y == 3.0).all())
    with pytest.raises(ValueError):
        preprocess_batch([np.zeros((1, 16385), np.uint8)], (64, 320), 1, True, augment=Augment())


def test_cli_train_with_augment(tmp_path):
    from img2latex_amd import cli
    config = {
        "model": {"name": "cnn_lstm", "embedding_dim": 32,
                  "encoder": {"cnn": {"img_height": 16, "img_width": 32, "channels": 1, "conv_filters": [4, 8, 16],
                                      "kernel_size": 3, "pool_size": 2, "padding": "same"}},
                  "decoder": {"hidden_dim": 64, "lstm_layers": 1, "dropout": 0.1, "attention": False, "max_seq_length": 20}},
        "data": {"batch_size": 4, "max_seq_length": 20},
        "training": {"device": "cuda", "epochs": 1, "learning_rate": 1e-3, "weight_decay": 0.0, "accumulation_steps": 1},
    }
    path = tmp_path / "config.yaml"
    path.write_text(yaml.safe_dump(config))
    kw = dict(synthetic_steps=2, synthetic_vocab=50, output_dir=str(tmp_path / "outputs"))
    out = cli.train(str(path), "aug", None, None, "cuda", 7, augment=True, **kw)
    assert out["steps"] == 2 and np.isfinite(out["loss"])
    plain = cli.train(str(path), "plain", None, None, "cuda", 7, **kw)
    assert np.isfinite(plain["loss"]) and plain["loss"] != out["loss"]       # the warp reached the batches
