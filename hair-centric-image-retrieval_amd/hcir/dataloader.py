"""hcir.dataloader — the reference's annotation-CSV dataset contract, host side only.

Contract kept (HP/utils/dataloader.py:13-41): `CustomDataset(annotations_file, img_dir,
transform=None, our_method=False)`; the CSV's first column is a file name relative to
`img_dir`, the second an integer class; an item is `(transform(image), label)`, or the dict
`{"anchor", "pos1"}` of a two-view transform when `our_method` is set.  Decoding uses PIL
(torchvision.io is not a dependency).

`EncodedDataset` + `collate_encoded` are the device-decode form of the same contract: the
workers only READ the files and stage them (`hcir.jpeg.stage_batch`: marker walk + unstuffing copy into
one blob); the batch that reaches the engine is a `StagedBatch`, which `Classifier._embed` uploads and decodes
with `hcir_png_decode_window_u8` (the reference's `*_hair.png` crops, `HP/data/data_train.csv`) or
`hcir_jpeg_decode_window_u8` (its `*_full_face` JPEG lists) -> `hcir_knn_transform_u8`.  Files outside both device
subsets (progressive JPEG, 16-bit or interlaced PNG ...) are decoded by the worker with PIL, as the reference does,
and ride along as RGB8 windows.

`collate_train_views` is the training side of the same contract: the items of an `EncodedDataset` become the two
SimCLR views the pretrain step consumes (`{"anchor", "pos1"}`, HP/utils/dataloader.py:36-38), with the whole-image
decode, the crops and the augmentations on the device (`hcir.views`).
"""
from __future__ import annotations

import csv
from pathlib import Path
from typing import Callable, List, Optional, Tuple

from PIL import Image
from torch.utils.data import Dataset


def _read_annotations(path: str) -> List[Tuple[str, int]]:
    """[(file name, class id)] from a header-ed two-column CSV (`id,class`)."""
    records: List[Tuple[str, int]] = []
    with open(path, newline="") as handle:
        reader = csv.reader(handle)
        next(reader, None)  # header row
        for row in reader:
            if len(row) >= 2 and row[0]:
                records.append((row[0], int(float(row[1]))))
    return records


class CustomDataset(Dataset):
    def __init__(self, annotations_file, img_dir, transform: Optional[Callable] = None, our_method=False):
        self.records = _read_annotations(annotations_file)
        self.root = Path(img_dir)
        self.transform = transform
        self.our_method = bool(our_method)

    def __len__(self) -> int:
        return len(self.records)

    def _decode(self, name: str) -> Image.Image:
        with Image.open(self.root / name) as im:
            return im.convert("RGB")

    def __getitem__(self, index: int):
        name, label = self.records[index]
        views = self.transform(self._decode(name)) if self.transform else self._decode(name)
        if self.our_method:
            first, second = views
            return {"anchor": first, "pos1": second}
        return views, label


class EncodedDataset(Dataset):
    """Same CSV contract as CustomDataset; an item is (file bytes as a uint8 tensor, label), with return_names
    (file bytes, label, file name) so that a collate function can name a corrupt file."""

    def __init__(self, annotations_file, img_dir, return_names: bool = False):
        self.records = _read_annotations(annotations_file)
        self.root = Path(img_dir)
        self.return_names = bool(return_names)

    def __len__(self) -> int:
        return len(self.records)

    def __getitem__(self, index: int):
        import numpy as np
        import torch
        name, label = self.records[index]
        data = torch.from_numpy(np.fromfile(self.root / name, dtype=np.uint8))
        return (data, label, name) if self.return_names else (data, label)


class EncodedBatch:
    """What collate_encoded hands to the engine: one staging blob per codec (JPEG files, PNG files) with the batch
    positions they fill, plus host-decoded windows of the files neither device decoder takes."""

    def __init__(self, parts, host_windows, size, n):
        self.parts, self.host_windows, self.size, self.n = parts, host_windows, size, n

    @property
    def staged(self):  # the single-codec batch's blob (kept for callers that look at sizes / bytes)
        return self.parts[0][1] if len(self.parts) == 1 else None

    def decode(self, device, check_status: bool = True):
        """-> uint8 [B, size, size, 3] on `device` (device decode; host-decoded files' windows copied in).
        check_status: read the decoders' per-image status back (one 4 B/image D2H per batch) and raise on a corrupt
        stream, as the reference's decode_image / PIL raise for the same file."""
        import torch
        from . import jpeg, png
        from ._lib import HcirError
        out = None
        for kind, staged, idx in self.parts:
            mod = jpeg if kind == "jpeg" else png
            try:
                win = mod.decode_windows(staged.to(device), self.size, check_status=check_status,
                                         _skip_rejected_check=True)
            except HcirError as e:
                raise HcirError(f"{e} (batch positions of this codec's files: {idx})") from None
            if len(self.parts) == 1 and len(idx) == self.n:
                out = win
            else:
                if out is None:
                    out = torch.zeros((self.n, self.size, self.size, 3), dtype=torch.uint8, device=device)
                out[torch.as_tensor(idx, device=device)] = win
        if out is None:
            out = torch.zeros((self.n, self.size, self.size, 3), dtype=torch.uint8, device=device)
        for i, win in self.host_windows.items():
            out[i].copy_(win, non_blocking=True)
        return out


def collate_encoded(items, size: int = 224, verify_crc: bool = True):
    """DataLoader collate_fn for EncodedDataset: (EncodedBatch, labels).  PNG files (the reference's *_hair.png
    crops) and baseline JPEGs are staged for their device decoders; anything else is decoded here with PIL."""
    import torch
    from . import jpeg, png
    files = [it[0] for it in items]
    is_png = [png.is_png(f) for f in files]
    parts, host = [], {}
    for kind, mod, sel in (("png", png, [i for i, p in enumerate(is_png) if p]),
                           ("jpeg", jpeg, [i for i, p in enumerate(is_png) if not p])):
        if not sel:
            continue
        sub = [files[i] for i in sel]
        # a worker is one process: its own core
        staged = mod.stage_batch(sub, pin=False, threads=1, verify_crc=verify_crc) if kind == "png" else \
            mod.stage_batch(sub, pin=False, threads=1)
        for j in staged.rejected:
            host[sel[j]] = jpeg.host_window(sub[j], (size, size))
        if len(staged.rejected) < len(sub):
            parts.append((kind, staged, sel))
    return EncodedBatch(parts, host, size, len(files)), torch.as_tensor([int(it[1]) for it in items])


class TrainViewBatch:
    """What collate_train_views hands to the trainer: per (codec, height, width) group one staging blob with the batch
    positions it fills, the host-decoded images of the files neither device decoder takes, and the labels."""

    def __init__(self, groups, host_images, names, labels):
        self.groups, self.host_images, self.names, self.labels = groups, host_images, names, labels
        self.n = len(names)

    def images(self, device):
        """-> (list of n RGB8 [h, w, 3] tensors on `device`, check): every staged file decoded whole on the device
        (one H2D copy per blob).  check() reads the decoders' status back (one copy for the batch) and raises
        HcirError naming the corrupt files; call it after enqueuing the work that follows."""
        import torch
        from . import jpeg, png
        from ._lib import HcirError
        images = [None] * self.n
        statuses, where = [], []
        for kind, (h, w), staged, idx, keep in self.groups:
            mod = png if kind == "png" else jpeg
            whole, st = mod.decode_windows(staged.to(device), (h, w), _skip_rejected_check=True, return_status=True)
            for k in keep:   # a rejected file's position in the blob is left alone by the device: PIL decoded it
                images[idx[k]] = whole[k]
            statuses.append(st if len(keep) == len(idx) else st[keep])
            where += [idx[k] for k in keep]
        for i, img in self.host_images.items():
            images[i] = img.to(device, non_blocking=True)
        if not statuses:
            return images, lambda: None
        st = torch.cat(statuses) if len(statuses) > 1 else statuses[0]
        st_host = torch.empty(st.shape, dtype=st.dtype, pin_memory=True)
        st_host.copy_(st, non_blocking=True)
        read = torch.cuda.Event()
        read.record(torch.cuda.current_stream(device))

        def check():
            read.synchronize()
            bad = [self.names[where[j]] for j in torch.nonzero(st_host).flatten().tolist()]
            if bad:
                raise HcirError(f"corrupt image data in files {bad}")

        return images, check

    def views(self, device, generator=None, boxes=None, params=None, defer_check: bool = False, **transform_kwargs):
        """-> {"anchor", "pos1"} fp32 [n, 3, 224, 224] on `device` (hcir.views.simclr_views over the decoded images).
        A corrupt stream raises HcirError with the file names: it never yields a black image.  defer_check: return
        (views, check) without waiting for the device; the caller runs check() before it trusts the batch (a producer
        on a side stream calls it after it has enqueued the step that runs beside)."""
        from . import views
        images, check = self.images(device)
        out = views.simclr_views(images, generator, boxes, params, **transform_kwargs)
        if defer_check:
            return out, check
        check()
        return out


def collate_train_views(items, verify_crc: bool = True, chunk: int = 256, threads: int = 1, pin: bool = False):
    """DataLoader collate_fn for EncodedDataset -> TrainViewBatch.  PNG files (the reference's *_hair.png crops) and
    baseline JPEGs are staged for their device decoders, per (codec, size) group and at most `chunk` files per blob
    (the decoders' workspace is about 3 bytes per pixel and file); anything else is decoded here with PIL, file by
    file, as the reference does.  threads / pin: for a caller that collates in the main process (a worker is one
    process: its own core, and its blobs are pinned by the DataLoader)."""
    import io

    import numpy as np
    import torch
    from . import jpeg, png
    from ._lib import HcirError
    from .hair_encoder import _sniff
    files = [jpeg._as_u8(it[0]) for it in items]
    names = [str(it[2]) if len(it) > 2 else f"<batch position {i}>" for i, it in enumerate(items)]
    by_group = {}
    for i, a in enumerate(files):
        by_group.setdefault(_sniff(a), []).append(i)
    groups, host = [], {}

    def host_image(i):
        try:
            with Image.open(io.BytesIO(files[i].tobytes())) as im:
                return torch.from_numpy(np.asarray(im.convert("RGB")).copy())
        except Exception as e:  # PIL's error for a file it cannot decode, with the file's name
            raise HcirError(f"cannot decode {names[i]}: {e}") from None

    for (kind, h, w), idx in by_group.items():
        if kind == "host":
            for i in idx:
                host[i] = host_image(i)
            continue
        mod = png if kind == "png" else jpeg
        for s in range(0, len(idx), max(int(chunk), 1)):
            sel = idx[s:s + max(int(chunk), 1)]
            sub = [files[i] for i in sel]
            staged = mod.stage_batch(sub, pin=pin, threads=threads, verify_crc=verify_crc) if kind == "png" else \
                mod.stage_batch(sub, pin=pin, threads=threads)
            rejected = set(staged.rejected)   # outside the device subset, or no valid file at all: PIL decides
            for j in rejected:
                host[sel[j]] = host_image(sel[j])
            keep = [j for j in range(len(sel)) if j not in rejected]
            if keep:
                groups.append((kind, (h, w), staged, sel, keep))
    return TrainViewBatch(groups, host, names, torch.as_tensor([int(it[1]) for it in items]))
