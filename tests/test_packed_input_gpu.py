"""Packed uint8 data set on the device: the three input kernels bit for bit against the float32 path, whole
training steps fused against unfused and resident against streamed, slot recycling of the streamed ring, and the CLI.

Reference arithmetic.  The contract is the HOST expression of the folder loader (`data_rescale` / `soft` on CPU float32
tensors: a correctly rounded division by 127.5f, tests/test_packed_input_cpu.py), so the expected values are computed
with torch ON THE CPU and compared with what the kernels wrote.  torch's device division by a Python scalar multiplies by
the rounded reciprocal and differs from it for 111 of the 256 byte values; it is not the reference."""
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from littlegan_amd.utils import data_rescale, soft

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rows(N, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    src = torch.randint(0, 256, (N, H, W, 3), dtype=torch.uint8, generator=g)
    src[0, 0, 0] = 77                      # a grey pixel: the hue rotation must pass it through
    src.view(-1)[:256] = torch.arange(256, dtype=torch.uint8)      # every byte value is present
    return src


def _gather(N, B, seed):
    """a permuted index vector with repeats, B entries into N rows"""
    g = torch.Generator().manual_seed(seed)
    idx = torch.randperm(N, generator=g)[:B] if B <= N else torch.randint(0, N, (B,), generator=g)
    idx = idx.clone()
    if B > 2:
        idx[B // 2] = idx[0]               # a repeated row
    return idx.to(torch.int64)


@pytest.mark.parametrize("N,B,shape", [(7, 5, (8, 8, 3)), (300, 256, (128, 128, 3)), (20, 16, (256, 256, 3)),
                                        (9, 6, (5, 7, 3)), (4, 3, (1, 1, 17))])
def test_rescale_u8_is_the_host_expression(N, B, shape):
    """8x8 (row_elems = 192), 128x128 at B=256 and 256x256 at B=16 take the 16-byte path; 5x7x3 = 105 and 17 bytes per row are
    not multiples of 16 and take the one-element-per-thread path (the tail)."""
    from littlegan_amd import ops
    g = torch.Generator().manual_seed(N)
    src = torch.randint(0, 256, (N,) + shape, dtype=torch.uint8, generator=g)
    src.view(-1)[:min(256, src.numel())] = torch.arange(min(256, src.numel()), dtype=torch.uint8)
    idx = _gather(N, B, 1)
    got = ops.rescale_u8(src.cuda(), idx.cuda()).cpu()
    exp = data_rescale(src[idx].float())
    assert got.shape == exp.shape and torch.equal(got, exp)
    # an unaligned source (a view one byte into a buffer) must take the scalar path and still be exact
    if shape == (8, 8, 3):
        buf = torch.zeros(src.numel() + 16, dtype=torch.uint8, device="cuda")
        buf[1:1 + src.numel()] = src.view(-1).cuda()
        off = buf[1:1 + src.numel()].view(src.shape)
        assert off.data_ptr() % 16 == 1 and torch.equal(ops.rescale_u8(off, idx.cuda()).cpu(), exp)


@pytest.mark.parametrize("N,B,A,cols", [(50, 8, 3, [0, 2]), (300, 256, 40, [8, 15, 20, 22, 26, 36, 39]), (5, 7, 4, [3, 3, 0])])
def test_soft_labels_is_the_host_expression(N, B, A, cols):
    from littlegan_amd import ops
    g = torch.Generator().manual_seed(B)
    attr = torch.randint(-1, 2, (N, A), generator=g).float()
    attr[0, 0] = 0.3                       # not only -1, 0, 1
    idx = _gather(N, B, 2)
    got = ops.soft_labels(attr.cuda(), idx.cuda(), torch.tensor(cols, dtype=torch.int32, device="cuda")).cpu()
    assert torch.equal(got, soft(attr[idx][:, cols]))


def _flips(B, seed, draw_offset):
    from oracle import input_oracle as I
    return np.asarray(I.step_draws(B, seed, draw_offset)[3]).astype(bool)


@pytest.mark.parametrize("N,B,H,W", [(300, 256, 128, 128), (20, 16, 64, 64), (6, 4, 6, 10), (5, 3, 8, 12)])
@pytest.mark.parametrize("noise_scale", [0.0, 0.02])
def test_augment_drawn_u8_is_augment_drawn_of_the_rescaled_rows(N, B, H, W, noise_scale):
    """Both outputs bit for bit, with and without out_rescaled.  6x10 has W % 4 != 0 (one pixel per thread), 8x12 and the
    two issue sizes take the 4-pixel path.  The seed is chosen by LOOKING at the drawn flips: the first of a fixed list whose
    window flips at least one image and leaves at least one alone."""
    from littlegan_amd import ops
    step = 7
    doff, noff = (step << 40) + (1 << 39), (step << 40) + (1 << 38)
    seed = next(s for s in [(k << 20) ^ 1 for k in range(1, 64)] if 0 < _flips(B, s, doff).sum() < B)
    flips = _flips(B, seed, doff)
    assert flips.any() and not flips.all()
    src = _rows(N, H, W, N + H)
    idx = _gather(N, B, 3)
    d_src, d_idx = src.cuda(), idx.cuda()
    rescaled = ops.rescale_u8(d_src, d_idx)
    assert torch.equal(rescaled.cpu(), data_rescale(src[idx].float()))
    exp = ops.augment_drawn(rescaled, 0.02, 0.75, 1.003, 0.03, noise_scale, seed, doff, noff)
    # d_in-style output: the first half of a [2B, H, W, 3] buffer, as the trainer passes it
    d_in = torch.full((2 * B, H, W, 3), float("nan"), device="cuda")
    aug, resc = ops.augment_drawn_u8(d_src, d_idx, 0.02, 0.75, 1.003, 0.03, noise_scale, seed, doff, noff, out=d_in[:B])
    torch.cuda.synchronize()
    assert aug.data_ptr() == d_in.data_ptr() and torch.equal(aug, exp) and torch.equal(resc, rescaled)
    assert torch.isnan(d_in[B:]).all()                                   # nothing written past the first half
    aug2, none = ops.augment_drawn_u8(d_src, d_idx, 0.02, 0.75, 1.003, 0.03, noise_scale, seed, doff, noff, want_rescaled=False)
    assert none is None and torch.equal(aug2, exp)
    # the flips really happened as drawn (noise off: a flipped image is mirrored up to the per-batch colour transform)
    if noise_scale == 0.0:
        plain = rescaled
        d_flip = (aug - plain.flip(2)).abs().amax((1, 2, 3)).cpu().numpy()
        d_keep = (aug - plain).abs().amax((1, 2, 3)).cpu().numpy()
        assert ((d_flip < d_keep) == flips).all()


# ---------------------------------------------------------------------------------------------------- whole steps
def _write_pack(path, n, dim, n_attr, seed):
    """A pack written directly in its documented format (the packer itself is covered by the CPU tests)."""
    os.makedirs(path, exist_ok=True)
    rng = np.random.default_rng(seed)
    np.save(os.path.join(path, "images.npy"), rng.integers(0, 256, (n, dim, dim, 3), dtype=np.uint8))
    np.save(os.path.join(path, "attr.npy"), rng.choice([-1.0, 1.0], (n, n_attr)).astype(np.float32))
    with open(os.path.join(path, "meta.json"), "w") as f:
        json.dump({"version": 1, "n": n, "h": dim, "w": dim, "c": 3, "attr_columns": n_attr,
                   "files": [f"{i:06d}.png" for i in range(n)]}, f)


def _trainer(cfg, W, pack, **kw):
    from littlegan_amd.dataset import CelebA
    from test_step_gpu import build
    tr = build(cfg, W, "bf16")
    a = tr.args
    a.image_dim, a.attr, a.packed_path, a.prefetch_batch, a.fuse_input, a.data_resident = cfg.image_dim, [0, 2, 3], pack, 3, True, True
    for k, v in kw.items():
        setattr(a, k, v)
    tr.dataset = CelebA(a)
    return tr


def _run_steps(tr, steps):
    it = tr.dataset.get_new_iterator()
    out = []
    for b in range(1, steps + 1):
        r = tr._train_step(b, it)
        assert r[0] is True, (b, r)
        out.append(r[1:])
    torch.cuda.synchronize()
    return out


def _same(tr_a, out_a, tr_b, out_b):
    for b, (ra, rb) in enumerate(zip(out_a, out_b), 1):
        for x, y in zip(ra, rb):
            assert (x is None) == (y is None) and (x is None or torch.equal(x, y)), b
    assert out_a[10][1] is not None                                       # the Adjuster branch ran at step 11
    for x, y in ((tr_a.store.flat, tr_b.store.flat), (tr_a.store.m, tr_b.store.m), (tr_a.store.v, tr_b.store.v)):
        assert torch.equal(x, y)


@pytest.mark.parametrize("other", [dict(fuse_input=False), dict(data_resident=False), dict(data_resident=False, fuse_input=False)])
def test_twelve_steps_are_bit_equal(tmp_path, other):
    """fuse_input on against off, resident against streamed: 12 _train_step calls (partition steps 5 and 10, the Adjuster
    branch from step 11) leave bit-equal parameters, Adam slots and returned images / losses."""
    from oracle import np_oracle as O
    from test_step_gpu import perturbed
    cfg = O.Cfg(init_dim=2, conv_filter=(64, 32, 32, 64, 32), cond_dim=3, noise_dim=11, batch_size=3)
    W = perturbed(cfg, 5)
    pack = str(tmp_path / "pack")
    _write_pack(pack, 26 * cfg.batch_size + 1, cfg.image_dim, 5, seed=1)          # 26 batches: 12 steps and one to spare
    tr_a, tr_b = _trainer(cfg, W, pack), _trainer(cfg, W, pack, **other)
    assert tr_a.dataset.resident and tr_b.dataset.resident == other.get("data_resident", True)
    _same(tr_a, _run_steps(tr_a, 12), tr_b, _run_steps(tr_b, 12))
    # the epoch ends at the same place on both: 26 batches = 13 steps, then out of range
    it = tr_a.dataset.get_new_iterator()
    assert [tr_a._train_step(b, it)[0] for b in range(1, 15)] == [True] * 13 + [None]


@pytest.mark.parametrize("prefetch", [1, 3])
def test_streamed_ring_yields_the_resident_batches(tmp_path, prefetch):
    """More batches than slots (10 batches: every slot of a ring of 1 or 3 is reused at least twice), each batch compared
    with resident mode only AFTER the whole epoch has been enqueued, so a slot refilled before its consumer kernel had
    read it would show up as a wrong earlier batch.  One run, no repetition."""
    from littlegan_amd.dataset import CelebA
    B, dim = 64, 64
    pack = str(tmp_path / "pack")
    _write_pack(pack, 10 * B, dim, 4, seed=2)
    base = dict(image_path="", attr_path="", image_ext="png", image_dim=dim, image_channel=3, attr=[1, 3], batch_size=B,
                device="cuda", seed=5, synthetic=False, threads=4, packed_path=pack)
    res = CelebA(SimpleNamespace(**base, data_resident=True, prefetch_batch=prefetch))
    stream = CelebA(SimpleNamespace(**base, data_resident=False, prefetch_batch=prefetch))
    assert res.resident and not stream.resident and res.batches == stream.batches == 10
    it_r, it_s = res.get_new_iterator(), stream.get_new_iterator()
    got_r = [it_r.get_next() for _ in range(10)]
    got_s = [it_s.get_next() for _ in range(10)]
    for it in (it_r, it_s):
        with pytest.raises(StopIteration):
            it.get_next()
    torch.cuda.synchronize()
    images = np.load(os.path.join(pack, "images.npy"))
    for k, ((ir, cr), (is_, cs)) in enumerate(zip(got_r, got_s)):
        assert torch.equal(ir, is_) and torch.equal(cr, cs), k
        b = it_r.order[k]
        assert torch.equal(ir.cpu(), data_rescale(torch.from_numpy(images[b * B:(b + 1) * B]).float())), k
    import threading
    assert not [t for t in threading.enumerate() if t.name == "littlegan-pack-stream"]


def test_cli_pack_then_train(tmp_path):
    """`main.py pack` then `main.py train` on that pack, each in a fresh child process under a time limit."""
    from PIL import Image
    dim, B, n = 32, 4, 4 * 24 + 1
    (tmp_path / "img").mkdir()
    rng = np.random.default_rng(0)
    rows = []
    for i in range(n):
        Image.fromarray(rng.integers(0, 256, (dim, dim, 3), dtype=np.uint8), "RGB").save(tmp_path / "img" / f"{i:05d}.png")
        rows.append(f"{i:05d}.png " + " ".join(str(v) for v in rng.choice([-1, 1], 4)))
    (tmp_path / "attr.txt").write_text("\n".join(rows) + "\n")
    cfgdir, res = tmp_path / "cfg", tmp_path / "results"
    cfgdir.mkdir()
    (cfgdir / "sample.config.json").write_text("{}")
    (cfgdir / "t.config.json").write_text(json.dumps({
        "image_path": str(tmp_path / "img"), "attr_path": str(tmp_path / "attr.txt"), "image_ext": "png", "attr": [0, 1, 3],
        "packed_path": str(tmp_path / "pack"), "threads": 4, "all_result_dir": str(res), "test_data_dir": str(tmp_path / "td"),
        "batch_size": B, "epoch": 1, "freq_gen": 4, "freq_test": 1000, "mfma_dtype": "bf16", "train_adj": True, "image_dim": dim,
        "init_dim": 2, "conv_filter": [64, 32, 32, 32, 32], "noise_dim": 7, "restore": False}))
    env = dict(os.environ, LITTLEGAN_CONFIG_DIR=str(cfgdir))

    def run(mode):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "main.py"), mode, "exp", "-e", "t", "--debug"], env=env,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (mode, r.stdout[-2000:], r.stderr[-2000:])
        return r.stdout

    assert "packed %d images" % n in run("pack")
    assert np.load(tmp_path / "pack" / "images.npy", mmap_mode="r").shape == (n, dim, dim, 3)
    out = run("train")
    assert "Epoch: 1" in out and "LossG" in out
    assert (res / "exp" / "checkpoint" / "ckpt-1.pt").is_file() and (res / "exp" / "train" / "gen" / "1-12.jpg").is_file()
