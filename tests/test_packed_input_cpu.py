"""Packed uint8 data set, host side: the pack round trip, batch-for-batch equality with the folder loader
(one rank and two), the exactness of the host arithmetic, the C ABI of the three new entry points and their argument
validation (no GPU needed: validation happens before any launch), and the life time of the streaming worker thread."""
import gc
import json
import os
import socket
import threading
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
from PIL import Image

from littlegan_amd.dataset import CelebA, pack_dataset
from littlegan_amd.utils import data_rescale, soft

B, DIM = 3, 8
THREAD_NAME = "littlegan-pack-stream"


def _args(root, **kw):
    d = dict(image_path=os.path.join(root, "img"), attr_path=os.path.join(root, "attr.txt"), image_ext="png", image_dim=DIM,
             image_channel=3, attr=[0, 2], batch_size=B, device="cpu", seed=3, synthetic=False, threads=4, prefetch_batch=2)
    d.update(kw)
    return SimpleNamespace(**d)


def _make_folder(root, n, seed=0):
    """n seeded PNGs (lossless) and a 3-column header-less attribute file; returns {file name: pixels}, {file name: labels}"""
    os.makedirs(os.path.join(root, "img"), exist_ok=True)
    rng = np.random.default_rng(seed)
    pix, lab, rows = {}, {}, []
    for i in range(n):
        a = rng.integers(0, 256, (DIM, DIM, 3), dtype=np.uint8)
        name = f"{i:04d}.png"
        Image.fromarray(a, "RGB").save(os.path.join(root, "img", name))
        pix[name] = a
        lab[name] = [int(v) for v in rng.choice([-1, 1], 3)]
        rows.append(name + " " + " ".join(str(v) for v in lab[name]))
    with open(os.path.join(root, "attr.txt"), "w") as f:
        f.write("\n".join(rows) + "\n")
    return pix, rows


def _streamers():
    return [t for t in threading.enumerate() if t.name == THREAD_NAME]


def test_pack_round_trip(tmp_path):
    root = str(tmp_path)
    n = 5 * B + 1
    pix, rows = _make_folder(root, n)
    a = _args(root)
    assert pack_dataset(a, os.path.join(root, "pack4")) == n
    images = np.load(os.path.join(root, "pack4", "images.npy"))
    attr = np.load(os.path.join(root, "pack4", "attr.npy"))
    meta = json.load(open(os.path.join(root, "pack4", "meta.json")))
    assert images.dtype == np.uint8 and images.shape == (n, DIM, DIM, 3)
    assert attr.dtype == np.float32 and attr.shape == (n, 3)                      # ALL columns, whatever args.attr says
    assert (meta["n"], meta["h"], meta["w"], meta["c"]) == (n, DIM, DIM, 3) and meta["version"] == 1
    # row order == the folder loader's file order; the pixels are the pixels written
    loader_files = [os.path.basename(p) for p in CelebA(a)._image_list]
    assert meta["files"] == loader_files and sorted(loader_files) == sorted(pix)
    for i, name in enumerate(meta["files"]):
        assert np.array_equal(images[i], pix[name])
    # attribute row i is line i of the file (the folder loader pairs file i with line i)
    assert np.array_equal(attr, np.asarray([[float(v) for v in r.split()[1:]] for r in rows], np.float32))
    # the result does not depend on the worker count
    pack_dataset(_args(root, threads=1), os.path.join(root, "pack1"))
    assert np.array_equal(np.load(os.path.join(root, "pack1", "images.npy")), images)
    assert np.array_equal(np.load(os.path.join(root, "pack1", "attr.npy")), attr)
    assert json.load(open(os.path.join(root, "pack1", "meta.json"))) == meta
    # a wrong-sized image is an error that names the file
    Image.fromarray(np.zeros((DIM, DIM + 1, 3), np.uint8), "RGB").save(os.path.join(root, "img", "9999.png"))
    with open(os.path.join(root, "attr.txt"), "a") as f:
        f.write("9999.png 1 1 1\n")
    with pytest.raises(ValueError, match="9999.png"):
        pack_dataset(a, os.path.join(root, "bad"))


def _epochs(ds, epochs=2):
    out = []
    for _ in range(epochs):
        it = ds.get_new_iterator()
        ep = []
        for _ in range(ds.batches):
            ep.append(it.get_next())
        with pytest.raises(StopIteration):
            it.get_next()
        out.append(ep)
    return out


@pytest.mark.parametrize("resident", [True, False, "auto"])
def test_same_batches_as_the_folder_loader(tmp_path, resident):
    root = str(tmp_path)
    _make_folder(root, 5 * B + 1)
    pack_dataset(_args(root), os.path.join(root, "pack"))
    folder = CelebA(_args(root))
    packed = CelebA(_args(root, packed_path=os.path.join(root, "pack"), data_resident=resident,
                          image_path=os.path.join(root, "nowhere")))     # the pack alone is read
    assert packed.packed and not packed.synthetic and packed.resident == (resident is True)
    assert (packed.n, packed.total_batches, packed.batches, packed.label) == (folder.n, folder.total_batches, folder.batches,
                                                                              folder.label)
    assert folder.batches == 5
    for ep_f, ep_p in zip(_epochs(folder), _epochs(packed)):
        for (img_f, cond_f), (img_p, cond_p) in zip(ep_f, ep_p):
            assert img_p.dtype == torch.float32 and img_p.shape == (B, DIM, DIM, 3) and cond_p.shape == (B, 2)
            assert torch.equal(img_f, img_p) and torch.equal(cond_f, cond_p)
    # the raw record: bytes + row indices + labels; data sets without a pack do not have it
    it = packed.get_new_iterator()
    raw = it.get_next_raw()
    assert raw.src.dtype == torch.uint8 and raw.idx.dtype == torch.int64 and raw.idx.shape == (B,)
    assert raw.src.shape[1:] == (DIM, DIM, 3) and raw.src.shape[0] == (packed.n if packed.resident else B)
    raw.release()
    it.close()
    assert not hasattr(folder.get_new_iterator(), "get_next_raw")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_worker(rank, world, port, root, out_q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.set_num_threads(2)
        ds = CelebA(_args(root, packed_path=os.path.join(root, "pack")))
        assert (ds.rank, ds.world) == (rank, world)
        it = ds.get_new_iterator()
        got = [tuple(t.numpy() for t in it.get_next()) for _ in range(ds.batches)]
        try:
            it.get_next()
            got = None   # must have raised
        except StopIteration:
            pass
        out_q.put((rank, ds.batches, got))
    finally:
        dist.destroy_process_group()


def test_two_ranks_split_the_epoch(tmp_path):
    root = str(tmp_path)
    _make_folder(root, 5 * B + 1)
    pack_dataset(_args(root), os.path.join(root, "pack"))
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, port, root, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict((r, (nb, got)) for r, nb, got in (q.get(timeout=300) for _ in range(2)))
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    single = _epochs(CelebA(_args(root, packed_path=os.path.join(root, "pack"))), 1)[0]   # same seed: the same permutation
    assert len(single) == 5 and res[0][0] == res[1][0] == 2       # batches = total_batches // world: the odd batch is dropped
    key = lambda img: img.tobytes()
    mine = [{key(img) for img, _ in res[r][1]} for r in range(2)]
    assert len(mine[0]) == len(mine[1]) == 2 and not (mine[0] & mine[1])               # disjoint
    # the ranks are dealt the permutation round-robin: together its first 4 batches, labels included
    for r in range(2):
        for k, (img, cond) in enumerate(res[r][1]):
            assert np.array_equal(img, single[2 * k + r][0].numpy()) and np.array_equal(cond, single[2 * k + r][1].numpy())


def test_host_arithmetic_is_exact():
    """The packed path on the host computes data_rescale / soft themselves, and those equal the IEEE single-precision
    expressions the kernels evaluate: a true division by 127.5f (not a product with a rounded reciprocal), then - 1.0f;
    the product 0.96f * x rounded, then + 0.02f."""
    u8 = np.arange(256, dtype=np.uint8)
    got = data_rescale(torch.from_numpy(u8).float())
    ieee = (u8.astype(np.float32) / np.float32(127.5)) - np.float32(1.0)
    assert got.dtype == torch.float32 and np.array_equal(got.numpy().view(np.uint32), ieee.view(np.uint32))
    recip = u8.astype(np.float32) * (np.float32(1.0) / np.float32(127.5)) - np.float32(1.0)
    assert int((recip.view(np.uint32) != ieee.view(np.uint32)).sum()) == 111          # why the kernels divide
    lab = np.asarray([-1.0, 0.0, 1.0], np.float32)
    s = soft(torch.from_numpy(lab))
    ref = (np.float32(0.96) * lab).astype(np.float32) + np.float32(0.02)
    assert s.dtype == torch.float32 and np.array_equal(s.numpy().view(np.uint32), ref.view(np.uint32))


def test_packed_cpu_path_uses_that_arithmetic(tmp_path):
    root = str(tmp_path)
    _make_folder(root, 2 * B)
    pack_dataset(_args(root), os.path.join(root, "pack"))
    images = np.load(os.path.join(root, "pack", "images.npy"))
    attr = np.load(os.path.join(root, "pack", "attr.npy"))
    ds = CelebA(_args(root, packed_path=os.path.join(root, "pack"), data_resident=True, attr=[2, 1]))
    it = ds.get_new_iterator()
    order = list(it.order)
    for b in order:
        img, cond = it.get_next()
        rows = slice(b * B, (b + 1) * B)
        assert torch.equal(img, data_rescale(torch.from_numpy(images[rows]).float()))
        assert torch.equal(cond, soft(torch.from_numpy(attr[rows][:, [2, 1]])))       # the filter is applied at load time


def test_new_entry_points_are_declared_bound_and_exported():
    from littlegan_amd.csrc.build import build
    build(verbose=False)
    from littlegan_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "littlegan_hip.h")).read()
    for name in ("lg_rescale_u8", "lg_soft_labels", "lg_augment_drawn_u8", "lg_augment_drawn_u8_workspace_bytes"):
        assert name in _lib.SIGNATURES and hasattr(lib, name) and (name + "(") in header
    assert lib.lg_abi_version() == 1
    assert lib.lg_augment_drawn_u8_workspace_bytes(256) == lib.lg_augment_drawn_workspace_bytes(256) >= 256 * 13


def test_argument_validation_needs_no_gpu():
    from littlegan_amd.csrc.build import build
    build(verbose=False)
    from littlegan_amd import _lib
    lib = _lib.load()
    p = 0x1000   # a non-null address that is never dereferenced: every call below is rejected before any launch
    err = lambda: lib.lg_last_error().decode()
    assert lib.lg_rescale_u8(0, p, 4, 192, p, 0) == -1 and "null" in err()
    assert lib.lg_rescale_u8(p, 0, 4, 192, p, 0) == -1
    assert lib.lg_rescale_u8(p, p, 4, 192, 0, 0) == -1
    assert lib.lg_rescale_u8(p, p, 0, 192, p, 0) == -1 and "B=0" in err()
    assert lib.lg_rescale_u8(p, p, -3, 192, p, 0) == -1
    assert lib.lg_rescale_u8(p, p, 4, 0, p, 0) == -1
    assert lib.lg_soft_labels(0, p, p, 4, 3, 2, p, 0) == -1 and "null" in err()
    assert lib.lg_soft_labels(p, p, 0, 4, 3, 2, p, 0) == -1
    assert lib.lg_soft_labels(p, p, p, 0, 3, 2, p, 0) == -1 and "B=0" in err()
    assert lib.lg_soft_labels(p, p, p, 4, 3, 0, p, 0) == -1
    ws = lib.lg_augment_drawn_u8_workspace_bytes(4)
    aug = lambda src, idx, out, resc, Bn, H, W, wsp, wsb: lib.lg_augment_drawn_u8(
        src, idx, out, resc, Bn, H, W, 0.02, 0.75, 1.003, 0.03, 0.02, 1, 1 << 39, 1 << 38, wsp, wsb, 0)
    assert aug(0, p, p, 0, 4, 8, 8, p, ws) == -1 and "null" in err()
    assert aug(p, 0, p, 0, 4, 8, 8, p, ws) == -1
    assert aug(p, p, 0, 0, 4, 8, 8, p, ws) == -1
    assert aug(p, p, p, 0, 4, 8, 8, 0, ws) == -1
    assert aug(p, p, p, 0, 0, 8, 8, p, ws) == -1 and "B=0" in err()
    assert aug(p, p, p, 0, 4, 0, 8, p, ws) == -1
    assert aug(p, p, p, 0, 4, 8, 8, p, ws - 1) == -1 and "workspace" in err()
    assert aug(p, p, p, p, 4, 8, 8, p, ws) == -1                                   # out_aug == out_rescaled


@pytest.mark.parametrize("prefetch", [1, 3])
def test_stream_worker_ends_with_the_epoch_and_with_the_iterator(tmp_path, prefetch):
    root = str(tmp_path)
    _make_folder(root, 6 * B)
    pack_dataset(_args(root), os.path.join(root, "pack"))
    ds = CelebA(_args(root, packed_path=os.path.join(root, "pack"), data_resident=False, prefetch_batch=prefetch))
    assert not ds.resident and not _streamers()
    it = ds.get_new_iterator()
    assert len(_streamers()) == 1                                                  # the worker runs ahead of get_next()
    for _ in range(ds.batches):
        it.get_next()
    with pytest.raises(StopIteration):
        it.get_next()
    assert not _streamers()                                                        # the epoch ended
    it = ds.get_new_iterator()
    it.get_next()
    it.get_next()
    assert len(_streamers()) == 1
    del it                                                                         # dropped half-way
    gc.collect()
    assert not _streamers()
    # a raw record still held by the consumer does not keep the worker alive either; holding every slot of the ring and
    # asking for more is an error, not a hang
    it = ds.get_new_iterator()
    held = [it.get_next_raw() for _ in range(prefetch)]
    with pytest.raises(RuntimeError, match="release"):
        it.get_next_raw()
    for r in held[1:]:
        r.release()
    raw = held[0]
    del it
    gc.collect()
    assert not _streamers()
    raw.release()
