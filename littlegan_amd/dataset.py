"""Mirror of /root/reference/dataset.py:7-49 (interface only: `.batches`, `.label`,
`.get_new_iterator().get_next() -> (image[B,H,W,3] in [-1,1], cond[B,cond_dim])`).  The JPEG pipeline is
host I/O outside the hot path; `synthetic=True` (or a missing image_path) yields
CelebA-shaped random batches resident on the device, which is what the metric is quoted on.

A PACKED data set is the fast way to train on real images: `pack_dataset` decodes the folder once into one
uint8 array, `CelebA(args)` with `packed_path` set keeps that array on the device (or streams it through a ring of pinned
buffers), and a batch is a row-index vector that the HIP input kernels gather, rescale and augment."""
import json
import os
import queue
import threading
from concurrent.futures import ThreadPoolExecutor
from glob import glob

import numpy as np
import torch

from .utils import data_rescale, soft


class _Iterator:
    def __init__(self, ds):
        self.ds, self.i = ds, 0
        self.order = ds._order()

    def get_next(self):
        if self.i >= len(self.order):
            raise StopIteration  # tf.errors.OutOfRangeError
        b = self.order[self.i]
        self.i += 1
        return self.ds._batch(b)


class CelebA:
    def __init__(self, args):
        print(" - Initializing Dataset...")
        self.args = args
        self.device = torch.device(getattr(args, "device", "cuda"))
        self.packed = bool(getattr(args, "packed_path", None))
        files = [] if self.packed else glob(os.path.join(args.image_path, "*." + args.image_ext)) if os.path.isdir(str(args.image_path)) else []
        self.synthetic = bool(getattr(args, "synthetic", False)) or not files
        self.label = list(args.attr)
        if self.packed:
            self.synthetic = False
            self._image_list, self._attributes_list = None, None
            self._open_pack(args.packed_path)
        elif self.synthetic:
            self.n = int(getattr(args, "synthetic_images", 64 * args.batch_size))
            self._image_list, self._attributes_list = None, None
        else:
            self._image_list = files
            self._attributes_list = self._get_attr_list(args.attr_path, args.attr)
            self.n = len(files)
        # data parallel: the (seeded, rank-independent) batch order is dealt round-robin to the ranks, every rank takes
        # the same number of batches per epoch (the gradient all-reduce needs matching step counts)
        d = torch.distributed
        self.rank, self.world = (d.get_rank(), d.get_world_size()) if (d.is_available() and d.is_initialized()) else (0, 1)
        self.total_batches = self.n // args.batch_size
        self.batches = self.total_batches // self.world
        self._gen = torch.Generator().manual_seed(int(getattr(args, "seed", 0)) + 17)

    @staticmethod
    def _get_attr_list(attr_file, attr_filter):  # dataset.py:36-46
        with open(attr_file) as f:
            raw = f.read().splitlines()
        out = []
        for item in raw:
            a = item.split()[1:]
            out.append(a if attr_filter is None else [a[x] for x in attr_filter])
        return out

    def _order(self):
        # dataset.py:21-22: batch THEN shuffle with a `prefetch`-sized buffer; a full permutation of batches here
        order = torch.randperm(self.total_batches, generator=self._gen).tolist()
        return order[self.rank::self.world][:self.batches]

    def _batch(self, b):
        a = self.args
        B, H = a.batch_size, a.image_dim
        if self.synthetic:
            g = torch.Generator().manual_seed(1000003 * b + 7)
            img = torch.rand(B, H, H, a.image_channel, generator=g) * 2 - 1
            cond = soft(2.0 * torch.randint(0, 2, (B, len(a.attr)), generator=g).float() - 1.0)
            return img.to(self.device), cond.to(self.device)
        from PIL import Image
        idx = range(b * B, (b + 1) * B)
        imgs = np.stack([np.asarray(Image.open(self._image_list[i]).convert("RGB"), np.float32) for i in idx])
        cond = np.asarray([[float(v) for v in self._attributes_list[i]] for i in idx], np.float32)
        return data_rescale(torch.from_numpy(imgs)).to(self.device), soft(torch.from_numpy(cond)).to(self.device)

    # ------------------------------------------------------------------ packed data set
    def _open_pack(self, path):
        """Opens <path>/{images.npy, attr.npy, meta.json} (pack_dataset) memory-mapped and decides where the bytes live:
        resident on the device (uploaded once, here) or streamed per batch by the iterator's worker thread."""
        a = self.args
        with open(os.path.join(path, "meta.json")) as f:
            meta = json.load(f)
        if meta.get("version") != PACK_VERSION:
            raise ValueError(f"{path}: pack format version {meta.get('version')} (this build reads {PACK_VERSION})")
        self._images = np.load(os.path.join(path, "images.npy"), mmap_mode="r")
        attr = np.load(os.path.join(path, "attr.npy"))
        n = int(meta["n"])
        if self._images.dtype != np.uint8 or self._images.shape != (n, meta["h"], meta["w"], meta["c"]) or attr.shape[0] != n:
            raise ValueError(f"{path}: images.npy / attr.npy do not match meta.json")
        if (meta["h"], meta["w"], meta["c"]) != (a.image_dim, a.image_dim, a.image_channel):
            raise ValueError(f"{path}: packed images are {meta['h']}x{meta['w']}x{meta['c']}, the configuration asks for "
                             f"{a.image_dim}x{a.image_dim}x{a.image_channel}")
        self.n = n
        cols = list(range(attr.shape[1])) if a.attr is None else [int(c) for c in a.attr]
        if not cols or min(cols) < 0 or max(cols) >= attr.shape[1]:
            raise ValueError(f"{path}: attr {cols} out of range for {attr.shape[1]} packed attribute columns")
        cuda = self.device.type == "cuda"
        resident = getattr(a, "data_resident", "auto")
        if isinstance(resident, str):
            if resident.lower() not in ("auto", "true", "false"):
                raise ValueError(f"data_resident: 'auto', true or false, not {resident!r}")
            # auto: resident if the images take at most half of the free device memory; on the host the memory map IS the
            # resident form, so auto streams there
            resident = (cuda and self._images.nbytes <= torch.cuda.mem_get_info(self.device)[0] // 2) \
                if resident.lower() == "auto" else resident.lower() == "true"
        self.resident = bool(resident)
        # the attribute table is small (CelebA: 202 599 x 40 floats = 32 MB): on the device in both modes, all columns
        self._attr = torch.from_numpy(np.ascontiguousarray(attr, np.float32)).to(self.device)
        self._cols = torch.tensor(cols, dtype=torch.int32, device=self.device)
        self._images_dev = self._upload(self._images) if self.resident else None

    def _upload(self, images):
        """The whole uint8 array to the device, once, in chunks through two pinned staging buffers; the only waits are on the
        event of the copy that last read the staging buffer about to be refilled (host code, no device-wide sync)."""
        if self.device.type != "cuda":
            return torch.from_numpy(np.array(images))
        n, row = images.shape[0], int(np.prod(images.shape[1:]))
        dev = torch.empty(images.shape, dtype=torch.uint8, device=self.device)
        rows = max(1, min(n, (64 << 20) // row))
        stage = [torch.empty((rows,) + images.shape[1:], dtype=torch.uint8).pin_memory() for _ in range(2)]
        done = [None, None]
        with torch.cuda.device(self.device):
            for k, r0 in enumerate(range(0, n, rows)):
                r1, s = min(n, r0 + rows), k % 2
                if done[s] is not None:
                    done[s].synchronize()
                np.copyto(stage[s].numpy()[:r1 - r0], images[r0:r1])
                dev[r0:r1].copy_(stage[s][:r1 - r0], non_blocking=True)
                done[s] = torch.cuda.Event()
                done[s].record()
            for e in done:   # the staging buffers are dropped on return: their last copies must have read them
                if e is not None:
                    e.synchronize()
        return dev

    def get_new_iterator(self):
        return _PackedIterator(self) if self.packed else _Iterator(self)


# ---------------------------------------------------------------------------------------------------- packed data set
PACK_VERSION = 1


def _decode(path_dim):
    from PIL import Image
    path, dim = path_dim
    a = np.asarray(Image.open(path).convert("RGB"), np.uint8)
    if a.shape != (dim, dim, 3):
        raise ValueError(f"{path}: decoded image is {a.shape[1]}x{a.shape[0]}x{a.shape[2]}, the pack needs {dim}x{dim}x3 "
                         "(images are never resized)")
    return a


def pack_dataset(args, out_dir, chunk=256):
    """Decodes the image folder ONCE into out_dir/images.npy (uint8 [N, H, W, 3], row i = file i of the folder loader's
    list), out_dir/attr.npy (float32 [N, A_all], every column of the attribute file) and out_dir/meta.json.  Host only."""
    files = glob(os.path.join(args.image_path, "*." + args.image_ext)) if os.path.isdir(str(args.image_path)) else []
    if not files:
        raise FileNotFoundError(f"no *.{args.image_ext} files under {args.image_path}")
    n, dim = len(files), int(args.image_dim)
    if int(getattr(args, "image_channel", 3)) != 3:
        raise ValueError("pack_dataset: 3-channel images only")
    rows = CelebA._get_attr_list(args.attr_path, None)
    if len(rows) < n:
        raise ValueError(f"{args.attr_path}: {len(rows)} attribute rows for {n} images")
    attr = np.asarray([[float(v) for v in r] for r in rows[:n]], np.float32)   # row i belongs to file i, as in CelebA._batch
    os.makedirs(out_dir, exist_ok=True)
    images = np.lib.format.open_memmap(os.path.join(out_dir, "images.npy"), mode="w+", dtype=np.uint8, shape=(n, dim, dim, 3))
    workers = max(1, min(int(getattr(args, "threads", 1)), 16))
    with ThreadPoolExecutor(max_workers=workers) as ex:   # map keeps the order: the result does not depend on the worker count
        for c0 in range(0, n, chunk):
            part = files[c0:c0 + chunk]
            images[c0:c0 + len(part)] = np.stack(list(ex.map(_decode, [(f, dim) for f in part])))
    images.flush()
    del images
    np.save(os.path.join(out_dir, "attr.npy"), attr)
    with open(os.path.join(out_dir, "meta.json"), "w") as f:
        json.dump({"version": PACK_VERSION, "n": n, "h": dim, "w": dim, "c": 3, "attr_columns": int(attr.shape[1]),
                   "files": [os.path.basename(p) for p in files]}, f)
    return n


class RawBatch:
    """What get_next_raw() hands out: `src` uint8 [N or B, H, W, 3], `idx` int64 [B] rows of src, `cond` float32 [B, cond_dim].
    A streamed batch occupies a slot of the ring: call release() once the kernels that read `src` are enqueued."""

    def __init__(self, src, idx, cond, on_release=None):
        self.src, self.idx, self.cond, self._on_release = src, idx, cond, on_release

    def release(self):
        if self._on_release is not None:
            self._on_release()
            self._on_release = None


class _Ring:
    """The streamed mode's state, owned by the worker thread and the iterator (the worker holds no reference to the
    iterator, so dropping the iterator ends the worker).  Slot s = pinned host buffer + device buffer + two events:
    `copied[s]` after the upload (the consumer's stream waits on it), `released[s]` after the consumer's kernels (the copy
    stream waits on it before the slot's next upload)."""

    def __init__(self, ds, order):
        a = ds.args
        self.images, self.order, self.B, self.device = ds._images, list(order), a.batch_size, ds.device
        self.cuda = self.device.type == "cuda"
        if self.cuda and self.device.index is None:   # the worker thread and the copy stream need the device by number
            self.device = torch.device("cuda", torch.cuda.current_device())
        k = max(1, int(getattr(a, "prefetch_batch", 1)))
        shape = (self.B,) + tuple(self.images.shape[1:])
        self.host = [torch.empty(shape, dtype=torch.uint8) for _ in range(k)]
        self.copied, self.released = [None] * k, [None] * k
        if self.cuda:
            self.host = [h.pin_memory() for h in self.host]
            self.dev = [torch.empty(shape, dtype=torch.uint8, device=self.device) for _ in range(k)]
            self.stream = torch.cuda.Stream(self.device)
            for d in self.dev:
                d.record_stream(self.stream)   # the allocator must not hand the buffer out again under a pending copy
        else:
            self.dev = self.host
        self.free, self.ready, self.stop, self.held = queue.Queue(), queue.Queue(), False, 0
        for s in range(k):
            self.free.put(s)
        self.thread = threading.Thread(target=self._work, name="littlegan-pack-stream", daemon=True)
        self.thread.start()

    def _work(self):
        try:
            if self.cuda:
                torch.cuda.set_device(self.device)
            for b in self.order:
                s = self.free.get()                       # blocks while the consumer holds every slot
                if s is None or self.stop:
                    return
                if self.copied[s] is not None:
                    self.copied[s].synchronize()          # the slot's previous upload has read the pinned buffer
                np.copyto(self.host[s].numpy(), self.images[b * self.B:(b + 1) * self.B])
                if self.cuda:
                    with torch.cuda.stream(self.stream):
                        if self.released[s] is not None:
                            self.stream.wait_event(self.released[s])   # the previous batch's kernels have read the device buffer
                        self.dev[s].copy_(self.host[s], non_blocking=True)
                        self.copied[s] = torch.cuda.Event()
                        self.copied[s].record(self.stream)
                self.ready.put((s, b))
            self.ready.put(None)
        except BaseException as e:   # handed to the consumer: a dead worker must not look like an empty queue
            self.ready.put(e)

    def take(self):
        if self.held >= len(self.host):   # the worker can never refill: waiting for it would hang, so say what is wrong
            raise RuntimeError(f"all {len(self.host)} slots of the streaming ring are held: release() a RawBatch before asking for the next")
        item = self.ready.get()
        if isinstance(item, BaseException):
            raise item
        s, b = item
        self.held += 1
        if self.cuda:
            torch.cuda.current_stream(self.device).wait_event(self.copied[s])
        return s, b

    def release(self, s):
        if self.cuda:
            self.released[s] = torch.cuda.Event()
            self.released[s].record(torch.cuda.current_stream(self.device))
        self.held -= 1
        self.free.put(s)

    def close(self):
        self.stop = True
        self.free.put(None)
        if self.thread is not threading.current_thread():
            self.thread.join()


class _PackedIterator:
    def __init__(self, ds):
        self.ds, self.i = ds, 0
        self.order = ds._order()
        self._ring = None if ds.resident or not self.order else _Ring(ds, self.order)
        self._arange = torch.arange(ds.args.batch_size, dtype=torch.int64, device=ds.device)

    def has_next(self):
        return self.i < len(self.order)

    def get_next_raw(self):
        if self.i >= len(self.order):
            self.close()
            raise StopIteration  # tf.errors.OutOfRangeError
        ds, B = self.ds, self.ds.args.batch_size
        b = self.order[self.i]
        rows = self._arange + b * B
        if self._ring is None:
            src, idx, rel = ds._images_dev, rows, None
        else:
            ring = self._ring
            s, got = ring.take()
            assert got == b
            src, idx, rel = ring.dev[s], self._arange, (lambda: ring.release(s))
        self.i += 1
        if ds.device.type == "cuda":
            from . import ops
            cond = ops.soft_labels(ds._attr, rows, ds._cols)
        else:
            cond = soft(ds._attr[rows][:, ds._cols.long()])
        if self.i >= len(self.order) and self._ring is not None:
            self._ring.thread.join()   # the worker has queued its last batch: the epoch leaves no thread behind
        return RawBatch(src, idx, cond, rel)

    def get_next(self):
        r = self.get_next_raw()
        if self.ds.device.type == "cuda":
            from . import ops
            img = ops.rescale_u8(r.src, r.idx)
        else:
            img = data_rescale(r.src[r.idx].float())
        r.release()
        return img, r.cond

    def close(self):
        if self._ring is not None:
            self._ring.close()
            self._ring = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
