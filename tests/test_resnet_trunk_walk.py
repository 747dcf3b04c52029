"""The ONE walk of ResNetEncoder's module tree behind its three trunk paths (bf16 eval, fp32 eval, training) and the ONE
cache of weight-derived images (packed bf16 filters, folded fp32 BatchNorm) behind the two eval paths.

(1) the launch sequence of every path against an expectation derived from the module tree alone; (2) a cold encoder
entered from two streams at once; (3) the cache's key rule.  Every comparison of values is ``torch.equal``: the paths are
deterministic, and what is compared is the same arithmetic on the same numbers."""
import pytest
import torch

from img2latex_amd import _lib, synth
from img2latex_amd.model import ResNetEncoder

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, H, W, E = 2, 32, 64, 16
PATHS = ["bf16", "fp32", "train"]


def _encoder(name, seed=5):
    enc = ResNetEncoder(H, W, 3, model_name=name, embedding_dim=E)
    shapes = [(k, tuple(v.shape)) for k, v in enc.state_dict().items()]
    np_sd = synth.make_resnet_state_dict(shapes, seed=seed)
    enc.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in np_sd.items()}, strict=True)
    return enc.to(DEV).eval()


def _fresh_like(enc):
    """A new encoder (empty caches) with the tensors `enc` holds now."""
    other = ResNetEncoder(H, W, 3, model_name=enc.model_name, embedding_dim=E)
    other.load_state_dict({k: v.detach().clone() for k, v in enc.state_dict().items()}, strict=True)
    other = other.to(DEV).eval()
    other.eval_precision, other.kernel_flags = enc.eval_precision, enc.kernel_flags
    return other


def _images(seed=9):
    return torch.from_numpy(synth.uniform(seed, "rimg", (B, 3, H, W), -1.0, 1.0)).to(DEV)


def _run(enc, path, x, joins=False):
    """The recorded launches of one pass as (conv, bn, x, residual, y, relu, nchw) tuples, and the tape (training)."""
    tape = None
    with torch.no_grad():
        if path == "train":
            enc.train()
            tape = {}
            enc._trunk_train(x, tape)
            recs = [(u["conv"], u["bn"], u["x"], u["residual"], u["y"], u["relu"], u["nchw"]) for u in tape["units"]]
        else:
            enc.eval()
            enc.eval_precision, enc.fuse_joins = path, joins
            enc.trace, enc.joined_heads = [], []
            enc.trunk(x)
            recs, enc.trace = enc.trace, None
    torch.cuda.synchronize()
    return recs, tape


def _check_sequence(enc, recs, x):
    """The expectation comes from the module tree: stem, then per block conv1, [conv2], [downsample], last unit.
    Returns per block (indices of the main units, index of the downsample or None), for the tape's ``blocks``."""
    m = enc.resnet
    conv, bn, xin, res, y, relu, nchw = recs[0]
    assert conv is m[0] and bn is m[1] and xin is x and res is None and relu is True and bool(nchw) is True
    stem_y = y
    i, block_in, out = 1, None, []
    for li in range(4, 8):
        for blk in m[li]:
            mains = [(blk.conv1, blk.bn1), (blk.conv2, blk.bn2)]
            if hasattr(blk, "conv3"):
                mains.append((blk.conv3, blk.bn3))
            main_idx, down_idx = [], None
            if block_in is None:                             # the first block reads the max-pool's output: not a unit
                block_in = recs[i][2]
                assert block_in is not stem_y and block_in is not x
                assert tuple(block_in.shape) == (B, (stem_y.shape[1] - 1) // 2 + 1, (stem_y.shape[2] - 1) // 2 + 1, 64)
            prev, identity = block_in, block_in
            for j, (c, b) in enumerate(mains):
                last = j == len(mains) - 1
                if last and blk.downsample is not None:      # the downsample sits in front of the last unit
                    conv, bn, xin, res, y, relu, nchw = recs[i]
                    assert conv is blk.downsample[0] and bn is blk.downsample[1], (li, i)
                    assert xin is block_in and res is None and relu is False and not nchw, (li, i)
                    identity, down_idx = y, i
                    i += 1
                conv, bn, xin, res, y, relu, nchw = recs[i]
                assert conv is c and bn is b, (li, i)
                assert xin is prev and relu is True and not nchw, (li, i)
                assert (res is identity) if last else (res is None), (li, i)
                main_idx.append(i)
                prev = y
                i += 1
            block_in = prev
            out.append((main_idx, down_idx))
    assert i == len(recs)
    return out


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", ["resnet18", "resnet50"])
def test_launch_sequence_follows_the_module_tree(name, path):
    enc, x = _encoder(name), _images()
    recs, tape = _run(enc, path, x)
    want_dtype = torch.bfloat16 if path == "bf16" else torch.float32
    assert all(r[4].dtype == want_dtype for r in recs)
    per_block = _check_sequence(enc, recs, x)
    assert enc.joined_heads == []
    if path == "train":
        blocks = tape["blocks"]
        assert len(blocks) == len(per_block)
        kind = "bottleneck" if name == "resnet50" else "basic"
        for rec, (main_idx, down_idx) in zip(blocks, per_block):
            assert rec["kind"] == kind and rec["main"] == main_idx and rec["down"] == down_idx
        assert tape["pool_in"] is recs[0][4] and tuple(tape["pool_shape"]) == tuple(recs[0][4].shape)
        assert tuple(tape["final_shape"]) == tuple(recs[-1][4].shape)


def test_joined_layer1_records_the_same_sequence():
    enc, x = _encoder("resnet50"), _images()
    recs, _ = _run(enc, "bf16", x, joins=True)
    _check_sequence(enc, recs, x)
    m = enc.resnet
    heads = [m[4][1].conv1, m[4][2].conv1, m[5][0].conv1]          # the three conv1 after layer1's blocks
    assert len(enc.joined_heads) == 3 and all(a is b for a, b in zip(enc.joined_heads, heads))


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_cold_cache_entered_from_two_streams(precision):
    """A pipeline with two encoder streams enters a cold encoder twice: the second stream hits the cache while the first
    stream's pack / fold kernels are still queued, and has to be ordered behind them."""
    x = _images()
    ref = _encoder("resnet18")
    ref.eval_precision = precision
    with torch.no_grad():
        want = ref.trunk(x)
    torch.cuda.synchronize()
    enc = _encoder("resnet18")
    enc.eval_precision = precision
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.no_grad():
        with torch.cuda.stream(sa):
            torch.cuda._sleep(20_000_000)                            # a few milliseconds in front of the pack kernels
            ya = enc.trunk(x)
        with torch.cuda.stream(sb):
            yb = enc.trunk(x)
    sa.synchronize()
    sb.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(ya, want), float((ya - want).abs().max())
    assert torch.equal(yb, want), float((yb - want).abs().max())


class _Count:
    """Counts the calls of the library's weight-image builders (the pack of the bf16 path, the fold of the fp32 path)."""
    NAMES = ("i2l_conv_bn_bf16_pack", "i2l_bn_eval_fold_f32")

    def __init__(self, monkeypatch):
        self.n = 0
        L = _lib.lib()
        for name in self.NAMES:
            monkeypatch.setattr(L, name, self._wrap(getattr(L, name)))

    def _wrap(self, fn):
        def call(*a):
            self.n += 1
            return fn(*a)
        return call


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_cache_rule(precision, monkeypatch):
    x = _images()
    enc = _encoder("resnet18")
    enc.eval_precision = precision
    count = _Count(monkeypatch)
    n_units = sum(isinstance(mod, torch.nn.Conv2d) for mod in enc.resnet.modules())

    def run(e):
        before = count.n
        with torch.no_grad():
            y = e.trunk(x)
        torch.cuda.synchronize()
        return y, count.n - before

    first, built = run(enc)
    assert built == n_units                                           # one image per conv unit
    again, built = run(enc)
    assert built == 0 and torch.equal(again, first)                   # cached
    with torch.no_grad():
        enc.resnet[5][0].conv1.weight.mul_(1.5)
    got, built = run(enc)
    assert built == (1 if precision == "bf16" else 0)                 # the fp32 kernels read the weight itself
    want, _ = run(_fresh_like(enc))
    assert torch.equal(got, want) and not torch.equal(got, first)
    enc.resnet[6][1].bn2.running_var.mul_(3.0)
    got2, built = run(enc)
    assert built == 1
    want2, _ = run(_fresh_like(enc))
    assert torch.equal(got2, want2) and not torch.equal(got2, got)
    enc.cache_packed_weights = False
    uncached, built = run(enc)
    assert built == n_units and torch.equal(uncached, got2)
    uncached, built = run(enc)
    assert built == n_units and torch.equal(uncached, got2)
