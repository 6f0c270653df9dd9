"""The data layer of the reference (processor/dataset.py:17-102) and a synthetic counterpart.

``MSDDataset`` reads the MVSA / HFM JSON + JPEG files with the reference's semantics and emits the 6-tuple
``(input_ids, input_mask, segment_ids, img_mask, label, image)``; its image is the DECODED uint8 RGB array, and ``ClipCollate``
(d2r_amd.image) packs a batch of them for the CLIP preprocessing kernel, which the trainer runs on the device.
``SyntheticMSDDataset`` emits the same tuple with a ready fp32 image.  Both go through the pinned-memory prefetching loader."""
from __future__ import annotations

import io
import json
import logging
import os

import numpy as np
import torch
from torch.utils.data import DataLoader, Dataset

from .jpeg import route

logger = logging.getLogger(__name__)


class MSDDataset(Dataset):
    """One split of an MVSA / HFM dataset (processor/dataset.py:17-102): `json_path` holds a list of {id, text, emotion_label},
    the image of sample `id` is ``<img_path>/<id>.jpg``.  Text: ``[CLS] + tokenize(text)[:max_seq - 2] + [SEP]`` as ids, zero
    padded to max_seq, mask 1 on the tokens, segment ids all 0; img_mask is 50 ones (unused by the model).  The image is opened
    with PIL and converted to RGB here (in the loader workers) and returned as a uint8 [H, W, 3] array; an image that cannot be
    opened is replaced by ``<img_path>/inf.png``, as in the reference, and counted.  `tokenizer` is a BertTokenizer or the
    directory / name to load one from (``do_lower_case=True``).  With ``image_decode="device"`` the workers only read the file:
    a JPEG that d2r_amd.jpeg.parse accepts is returned parsed (a JpegInfo, decoded on the GPU with the batch), any other file
    is decoded here as above.  ``labels_optional=True`` (prediction): an entry without ``emotion_label`` gets label -1 instead of
    raising.  ``ids`` keeps every entry's id, in file order."""

    def __init__(self, json_path: str, img_path: str, tokenizer, max_seq: int = 128, image_decode: str = "host",
                 labels_optional: bool = False):
        if image_decode not in ("host", "device"):
            raise ValueError(f"image_decode must be 'host' or 'device', got {image_decode!r}")
        self.image_decode = image_decode
        if isinstance(tokenizer, str):
            from transformers import BertTokenizer
            tokenizer = BertTokenizer.from_pretrained(tokenizer, do_lower_case=True)
        self.tokenizer, self.img_path, self.max_seq = tokenizer, img_path, max_seq
        with open(json_path, "r", encoding="utf-8") as f:
            data = json.load(f)
        self.texts = [s["text"] for s in data]
        if labels_optional:
            self.labels = [int(s["emotion_label"]) if s.get("emotion_label") is not None else -1 for s in data]
        else:
            self.labels = [int(s["emotion_label"]) for s in data]
        self.ids = [str(s["id"]) for s in data]
        self.imgs = [i + ".jpg" for i in self.ids]
        self.fallbacks = 0
        logger.info("loaded %d samples from %s", len(data), json_path)

    def __len__(self):
        return len(self.texts)

    def encode(self, text: str):
        tokens = ["[CLS]"] + self.tokenizer.tokenize(text)[:self.max_seq - 2] + ["[SEP]"]
        ids = self.tokenizer.convert_tokens_to_ids(tokens)
        pad = self.max_seq - len(ids)
        return (torch.tensor(ids + [0] * pad), torch.tensor([1] * len(ids) + [0] * pad), torch.zeros(self.max_seq, dtype=torch.long))

    def load_image(self, name: str):
        from PIL import Image
        try:
            if self.image_decode == "device":
                with open(os.path.join(self.img_path, name), "rb") as f:
                    data = f.read()
                info, _ = route(data)
                if info is not None:
                    return info
                with Image.open(io.BytesIO(data)) as im:
                    return np.asarray(im.convert("RGB"))
            with Image.open(os.path.join(self.img_path, name)) as im:
                return np.asarray(im.convert("RGB"))
        except Exception as e:  # the reference's bare `except:` (processor/dataset.py:91-95)
            self.fallbacks += 1
            logger.warning("image %s could not be read (%s): using inf.png (%d fallbacks in this process)", name, e, self.fallbacks)
            with Image.open(os.path.join(self.img_path, "inf.png")) as im:
                return np.asarray(im.convert("RGB"))

    def __getitem__(self, idx):
        ids, mask, seg = self.encode(self.texts[idx])
        img_mask = torch.ones(50, dtype=torch.long)
        return ids, mask, seg, img_mask, torch.tensor(self.labels[idx]), self.load_image(self.imgs[idx])


class SyntheticMSDDataset(Dataset):
    """Deterministic per-index samples: ids ~ U{1000..29999} with [CLS]=101 / [SEP]=102 / pad 0, ragged lengths,
    images ~ N(0,1) (what CLIPProcessor's normalisation produces), labels ~ U{0..C-1}; `learnable=True` plants a
    label-dependent offset in the image so that a short training run can show a falling loss."""

    def __init__(self, n: int, max_seq: int = 128, image_size: int = 224, num_classes: int = 3, seed: int = 0,
                 learnable: bool = True, num_image_tokens: int = 50):
        self.n, self.max_seq, self.image_size, self.num_classes = n, max_seq, image_size, num_classes
        self.seed, self.learnable, self.num_image_tokens = seed, learnable, num_image_tokens

    def __len__(self):
        return self.n

    @property
    def labels(self):
        """Every sample's label, in index order (the draws of __getitem__ up to the label, without the image)."""
        return [self._text_and_label(idx)[4] for idx in range(self.n)]

    def _text_and_label(self, idx):
        g = torch.Generator().manual_seed(self.seed * 1_000_003 + idx)
        L = self.max_seq
        length = int(torch.randint(max(L // 4, 3), L + 1, (1,), generator=g))
        ids = torch.zeros(L, dtype=torch.long)
        ids[:length] = torch.randint(1000, 30000, (length,), generator=g)
        ids[0], ids[length - 1] = 101, 102
        mask = torch.zeros(L, dtype=torch.long)
        mask[:length] = 1
        seg = torch.zeros(L, dtype=torch.long)
        label = int(torch.randint(0, self.num_classes, (1,), generator=g))
        return ids, mask, seg, g, label

    def __getitem__(self, idx):
        ids, mask, seg, g, label = self._text_and_label(idx)
        image = torch.randn(3, self.image_size, self.image_size, generator=g)
        if self.learnable:
            image = image + 0.5 * (label - (self.num_classes - 1) / 2.0)
            ids[1] = 2000 + label
        img_mask = torch.ones(self.num_image_tokens, dtype=torch.long)  # unused by the model (train.py:281-284)
        return ids, mask, seg, img_mask, torch.tensor(label), image


def make_loader(ds: Dataset, batch_size: int, shuffle: bool, num_workers: int = 0, drop_last: bool = False,
                sampler=None, collate_fn=None) -> DataLoader:
    """pin_memory + (optionally) worker processes, as run.py:131-140; H2D copies are issued non_blocking by the trainer."""
    return DataLoader(ds, batch_size=batch_size, shuffle=shuffle and sampler is None, num_workers=num_workers,
                      pin_memory=torch.cuda.is_available(), drop_last=drop_last, sampler=sampler,
                      persistent_workers=num_workers > 0, collate_fn=collate_fn)
