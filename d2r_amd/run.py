"""CLI counterpart of the reference's run.py (run.py:38-158): same flag names and defaults for everything the
model/trainer consume, plus the extensions of this build (--dtype, --num_classes, --synthetic sizes, data parallel via
torch.distributed.run).  Without --data_path the data is synthetic; with it, an MVSA / HFM directory is read
(MSDDataset) and the CLIP image preprocessing runs on the GPU (d2r_amd.image); --pretrained loads the BERT / CLIP checkpoints
of --bert_name / --vit_name (local directories) as the reference does (run.py:122-153):

    python -m d2r_amd.run --num_epochs 2 --batch_size 32 --train_samples 256
    python -m d2r_amd.run --data_path data/MVSA-single/10-flod-1 --img_path data/MVSA-single/MVSA_Single/data \
        --bert_name ./bert-base-uncased --vit_name ./clip-vit-base-patch32 --pretrained
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 -m d2r_amd.run --batch_size 256

--only_test --load_path <best_model.pth> predicts the test split with a saved checkpoint (no training; unlabelled test entries
allowed), --write_path writes the per-sample predictions as JSON Lines (MSDTrainer.predict); both are single-process.
--cache_dataset device (with --data_path) decodes every split once and serves all later batches from device memory (d2r_amd.cache).
--ema_decay D averages the weights inside the AdamW launch; the dev / test passes and best_model.pth use the average.
--label_smoothing E / --class_weights {none | balanced | W0,W1,...} are the options of the cross entropy (inside its kernels).
--focal_gamma G scales every sample's cross-entropy term by (1 - the probability of its target) ** G: the focal loss, inside the same
kernels' slot (d2r_ce_focal_*); it composes with the two options above, with MixUp / CutMix and with --dp_exact.
--aug_crop_scale LO / --aug_flip P (with --data_path) augment the training images on the device (d2r_amd.augment).
--aug_brightness B / --aug_contrast C / --aug_saturation S / --aug_hue H / --aug_grayscale P / --aug_erase P: the photometric half of
that augmentation (colour jitter in this fixed order, random grayscale, random erasing), in the same launch slot.
--layer_lr_decay D / --wd_exempt_1d / --weight_decay W: AdamW hyper-parameters per parameter, still one launch (d2r_adamw_step_table).
--drop_path P: stochastic depth of the two encoder towers, growing linearly with depth from 0 to P (d2r_drop_path), training only.
--aug_token_delete P / --aug_token_mask P / --aug_token_replace P / --aug_whole_word: per token of a training text, delete it, put
[MASK] in its place or replace it by a random id, per piece or per whole word, in the one launch that builds the batch's token
tensors on the device (d2r_token_augment, d2r_amd.text_augment); real and synthetic data.
--aug_mixup A / --aug_cutmix A / --aug_mix_prob P: MixUp / CutMix of the finished training pixel batch in one launch, with a cross
entropy against two labels per sample (d2r_image_mix, d2r_ce_mix_*, d2r_amd.mix); only the image is mixed; real and
synthetic data.
--patch_dropout P: PatchDropout of the vision tower: a training image keeps its class token and max(1, int(np * (1 - P))) of its np
patches, and everything behind the embedding runs on the shorter sequence (d2r_amd.patch_dropout); training only.
"""
from __future__ import annotations

import argparse
import contextlib
import logging
import math
import os
import random

import numpy as np
import torch

logging.basicConfig(format="%(asctime)s - %(levelname)s - %(name)s -   %(message)s", datefmt="%m/%d/%Y %H:%M:%S",
                    level=logging.INFO)
logger = logging.getLogger("d2r_amd.run")


def set_seed(seed=2023):
    torch.manual_seed(seed)
    torch.cuda.manual_seed_all(seed)
    np.random.seed(seed)
    random.seed(seed)


def _max_grad_norm(text):
    v = float(text)
    if not v >= 0:
        raise argparse.ArgumentTypeError(f"must be >= 0 (0 = no clipping), got {text}")
    return v


def _ema_decay(text):
    v = float(text)
    if not 0 <= v < 1:
        raise argparse.ArgumentTypeError(f"must be in [0, 1) (0 = no averaging), got {text}")
    return v


def _layer_lr_decay(text):
    v = float(text)
    if not 0 < v <= 1:
        raise argparse.ArgumentTypeError(f"must be in (0, 1] (1 = off), got {text}")
    return v


def _weight_decay(text):
    v = float(text)
    if not (v >= 0 and math.isfinite(v)):
        raise argparse.ArgumentTypeError(f"must be finite and >= 0, got {text}")
    return v


def _label_smoothing(text):
    v = float(text)
    if not 0 <= v < 1:
        raise argparse.ArgumentTypeError(f"must be in [0, 1) (0 = off), got {text}")
    return v


def _focal_gamma(text):
    v = float(text)
    if not (v >= 0 and math.isfinite(v)):
        raise argparse.ArgumentTypeError(f"must be finite and >= 0 (0 = off), got {text}")
    return v


def _aug_crop_scale(text):
    v = float(text)
    if not 0 < v <= 1:
        raise argparse.ArgumentTypeError(f"must be in (0, 1] (1 = no cropping), got {text}")
    return v


def _aug_flip(text):
    v = float(text)
    if not 0 <= v <= 1:
        raise argparse.ArgumentTypeError(f"must be in [0, 1] (0 = no flipping), got {text}")
    return v


def _aug_jitter(text):
    v = float(text)
    if not (v >= 0 and math.isfinite(v)):
        raise argparse.ArgumentTypeError(f"must be finite and >= 0 (0 = off), got {text}")
    return v


def _aug_hue(text):
    v = float(text)
    if not 0 <= v <= 0.5:
        raise argparse.ArgumentTypeError(f"must be in [0, 0.5] (0 = off), got {text}")
    return v


def _aug_token(text):
    v = float(text)
    if not 0 <= v <= 1:
        raise argparse.ArgumentTypeError(f"must be in [0, 1] (0 = off), got {text}")
    return v


def _aug_mix_alpha(text):
    v = float(text)
    if not (v >= 0 and math.isfinite(v)):
        raise argparse.ArgumentTypeError(f"must be finite and >= 0 (0 = off), got {text}")
    return v


def _aug_mix_prob(text):
    v = float(text)
    if not 0 <= v <= 1:
        raise argparse.ArgumentTypeError(f"must be in [0, 1], got {text}")
    return v


PHOTO_FLAGS = ("aug_brightness", "aug_contrast", "aug_saturation", "aug_hue", "aug_grayscale", "aug_erase")
_PHOTO_NAMES = " / ".join("--" + f for f in PHOTO_FLAGS)


TOKEN_FLAGS = ("aug_token_delete", "aug_token_mask", "aug_token_replace")
_TOKEN_NAMES = " / ".join("--" + f for f in TOKEN_FLAGS)
SYNTHETIC_TOKENS = dict(mask_id=103, pad_id=0, replace_range=(1000, 30000))  # SyntheticMSDDataset's ids: bert-base-uncased's layout


def token_settings(tokenizer, whole_word: bool, need_mask: bool):
    """TokenAugmenter's settings from a BertTokenizer: mask_id, pad_id, vocab = len(tokenizer), replace_range = (lo, vocab) with lo one
    past the largest id among the special tokens and the tokens spelled [unusedN], cont = continuation_table with `whole_word`.
    A tokenizer without a mask token is refused (SystemExit) when `need_mask`; its mask id is then the pad id (never written)."""
    import re
    from .text_augment import continuation_table
    if tokenizer.mask_token_id is None and need_mask:
        raise SystemExit("--aug_token_mask needs a tokenizer with a mask token: the one of --bert_name has none")
    if tokenizer.pad_token_id is None:
        raise SystemExit(f"{_TOKEN_NAMES} need a tokenizer with a padding token: the one of --bert_name has none")
    reserved = list(tokenizer.all_special_ids) + [i for t, i in tokenizer.get_vocab().items() if re.fullmatch(r"\[unused\d+\]", t)]
    vocab = len(tokenizer)
    lo = 1 + max(reserved)
    if lo >= vocab:
        raise SystemExit(f"{_TOKEN_NAMES}: the vocabulary of --bert_name holds no id past its special and [unusedN] tokens to replace by")
    mask_id = tokenizer.mask_token_id if tokenizer.mask_token_id is not None else tokenizer.pad_token_id
    return dict(mask_id=int(mask_id), pad_id=int(tokenizer.pad_token_id), vocab=vocab, replace_range=(lo, vocab),
                cont=continuation_table(tokenizer) if whole_word else None)


def _drop_path(text):
    v = float(text)
    if not 0 <= v < 1:
        raise argparse.ArgumentTypeError(f"must be in [0, 1) (0 = off), got {text}")
    return v


def _patch_dropout(text):
    v = float(text)
    if not (math.isfinite(v) and 0 <= v < 1):
        raise argparse.ArgumentTypeError(f"must be in [0, 1) (0 = off), got {text}")
    return v


def parse_class_weights(text, num_classes):
    """--class_weights: 'none' -> None, 'balanced' -> 'balanced' (resolved from the training split), 'W0,W1,...' -> the list of
    num_classes non-negative finite floats, not all zero.  Anything else: ValueError."""
    if text in ("none", "balanced"):
        return None if text == "none" else text
    try:
        w = [float(x) for x in text.split(",")]
    except ValueError:
        raise ValueError(f"--class_weights {text!r}: expected none, balanced or {num_classes} comma-separated numbers") from None
    if len(w) != num_classes:
        raise ValueError(f"--class_weights {text!r}: {len(w)} weights for --num_classes {num_classes}")
    if any(not np.isfinite(x) or x < 0 for x in w):
        raise ValueError(f"--class_weights {text!r}: every weight must be finite and >= 0")
    if not any(x > 0 for x in w):
        raise ValueError(f"--class_weights {text!r}: the weights are all zero (every loss would be 0 / 0)")
    return w


def balanced_class_weights(counts):
    """N / (C * n_c) from the per-class sample counts of the training split (sklearn's compute_class_weight("balanced")).  A class
    without a training sample has no such weight: ValueError naming it."""
    counts = [int(n) for n in counts]
    empty = [c for c, n in enumerate(counts) if n <= 0]
    if empty:
        raise ValueError(f"--class_weights balanced: class(es) {', '.join(map(str, empty))} have no sample in the training split "
                         f"(counts {counts}); give explicit weights instead")
    total, C = sum(counts), len(counts)
    return [total / (C * n) for n in counts]


def train_label_counts(args, train_json=None):
    """Per-class sample counts of the WHOLE training split (every rank sees all of it, not its shard): the labels of train.json, or
    of the synthetic training set."""
    if train_json is not None:
        import json
        with open(train_json, "r", encoding="utf-8") as f:
            labels = [int(s["emotion_label"]) for s in json.load(f)]
    else:
        from .data import SyntheticMSDDataset
        labels = SyntheticMSDDataset(args.train_samples, args.max_seq, args.image_size, args.num_classes, seed=1).labels
    bad = sorted({y for y in labels if not 0 <= y < args.num_classes})
    if bad:
        raise ValueError(f"training labels {bad} lie outside [0, {args.num_classes}) (--num_classes)")
    return np.bincount(np.asarray(labels, dtype=np.int64), minlength=args.num_classes).tolist()


def build_parser():
    p = argparse.ArgumentParser()
    # --- flags of the reference (run.py:39-84); unused ones are accepted and ignored like there
    p.add_argument("--bert_name", default="bert-base-uncased", type=str)
    p.add_argument("--vit_name", default="clip-vit-base-patch32", type=str)
    p.add_argument("--num_epochs", default=30, type=int)
    p.add_argument("--device", default="cuda", type=str)
    p.add_argument("--batch_size", default=32, type=int, help="GLOBAL batch (split over ranks under torch.distributed.run)")
    p.add_argument("--lr", default=3e-5, type=float)
    p.add_argument("--warmup_ratio", default=0.01, type=float)
    p.add_argument("--eval_begin_epoch", default=1, type=int)
    p.add_argument("--seed", default=2023, type=int)
    p.add_argument("--load_path", default=None, type=str)
    p.add_argument("--save_path", default="./output/", type=str)
    p.add_argument("--write_path", default=None, type=str, help="JSON Lines file of per-sample test-split predictions: the only pass "
                   "with --only_test, one pass with the best checkpoint after training otherwise")
    p.add_argument("--notes", default="", type=str)
    p.add_argument("--do_train", action="store_true", default=True)
    p.add_argument("--only_test", action="store_true", help="predict the test split with the --load_path checkpoint, no training")
    p.add_argument("--max_seq", default=128, type=int)
    p.add_argument("--ignore_idx", default=0, type=int)
    p.add_argument("--sample_ratio", default=1.0, type=float)
    p.add_argument("--alpha", default=0, type=float)
    p.add_argument("--margin", default=0.1, type=float)
    p.add_argument("--beta", default=0.1, type=float)
    p.add_argument("--mild_margin", default=0.7, type=float)
    p.add_argument("--hetero", default=0.9, type=float)
    p.add_argument("--homo", default=0.9, type=float)
    p.add_argument("--DR_step", default=3, type=int)
    p.add_argument("--weight_js_1", default=0.1, type=float)
    p.add_argument("--weight_js_2", default=0.1, type=float)
    p.add_argument("--weight_diff", default=0.1, type=float)
    p.add_argument("--embed_size", default=768, type=int)
    p.add_argument("--num_head_IMRC", type=int, default=16)
    p.add_argument("--hid_IMRC", type=int, default=768)
    p.add_argument("--raw_feature_norm_CMRC", default="clipped_l2norm")
    p.add_argument("--lambda_softmax_CMRC", default=4.0, type=float)
    p.add_argument("--hid_router", type=int, default=768)
    # --- extensions
    p.add_argument("--dtype", default="bf16", choices=["bf16", "fp16", "f32"])
    p.add_argument("--num_classes", default=3, type=int)
    p.add_argument("--num_cells", default=6, type=int, help="cells per routing layer: the first n of ric, glac, imrc, cmrc, "
                   "crcmc, gesc (6 = the reference; 2..5 = declared-subset extension, BASELINE configs[4] uses 4)")
    p.add_argument("--image_size", default=224, type=int)
    p.add_argument("--patch_size", default=32, type=int)
    p.add_argument("--encoder_layers", default=12, type=int)
    p.add_argument("--bert_dropout", default=0.1, type=float,
                   help="hidden_dropout_prob = attention_probs_dropout_prob of the BERT config (bert-base default 0.1)")
    p.add_argument("--train_samples", default=512, type=int)
    p.add_argument("--eval_samples", default=128, type=int)
    p.add_argument("--num_workers", default=4, type=int)
    p.add_argument("--max_grad_norm", default=0.0, type=_max_grad_norm, help="clip the gradient to this global L2 norm before every "
                   "AdamW step, as torch.nn.utils.clip_grad_norm_ would (0 = off, the reference's behaviour)")
    p.add_argument("--ema_decay", default=0.0, type=_ema_decay, help="keep an exponential moving average of the live weights, "
                   "updated inside the AdamW launch; the dev / test passes run on it and best_model.pth holds it (0 = off, the "
                   "reference's behaviour).  The decay warms up as torch_ema does with use_num_updates: step t uses "
                   "min(ema_decay, (1 + t) / (10 + t)), always, so a short run does not keep averaging its random initialisation")
    p.add_argument("--layer_lr_decay", default=1.0, type=_layer_lr_decay, help="layer-wise learning-rate decay of the two pretrained "
                   "towers (BEiT's convention): encoder layer i of L learns at D ** (L - i) of its group's rate, the embeddings at "
                   "D ** (L + 1), everything above the towers at the full rate; in (0, 1], 1 = off, the reference's behaviour")
    p.add_argument("--wd_exempt_1d", action="store_true", help="no weight decay on parameters with one dimension or none: biases, "
                   "LayerNorm / BatchNorm weight and bias, CLIP's class embedding (off = the reference's behaviour)")
    p.add_argument("--weight_decay", default=1e-2, type=_weight_decay, help="AdamW's decoupled weight decay, finite and >= 0 "
                   "(1e-2 = the reference's)")
    p.add_argument("--drop_path", default=0.0, type=_drop_path, help="stochastic depth (DropPath) of the two pretrained towers: in "
                   "training, encoder layer i of L drops each of its two residual branches per sample with probability P * i / (L - 1) "
                   "and scales it by the inverse of the rest otherwise (timm's / BEiT's linear schedule); in [0, 1), 0 = off, the "
                   "reference's behaviour; dev, test and prediction passes are never affected")
    p.add_argument("--patch_dropout", default=0.0, type=_patch_dropout, help="PatchDropout (Liu et al. 2022; open_clip's "
                   "--force-patch-dropout): in training, every image keeps its class token and K = max(1, int(np * (1 - P))) of its np "
                   "patches, drawn per sample, and the vision tower, the vision self layer and both routing modules run on 1 + K image "
                   "tokens (d2r_patchify_keep, d2r_clip_embed_finish_keep, d2r_clip_embed_bwd_keep); in [0, 1), 0 = off, the reference's "
                   "behaviour; dev, test and prediction passes always see all patches; real and synthetic data")
    p.add_argument("--label_smoothing", default=0.0, type=_label_smoothing, help="label smoothing of the cross entropy, in [0, 1), as "
                   "torch.nn.CrossEntropyLoss(label_smoothing=) (0 = off, the reference's behaviour); training, dev and test loss alike")
    p.add_argument("--class_weights", default="none", type=str, help="per-class weights of the cross entropy, as "
                   "torch.nn.CrossEntropyLoss(weight=): none (the reference's behaviour), balanced (N / (C * n_c) over the whole "
                   "training split) or --num_classes comma-separated numbers W0,W1,...; not with --dp_exact")
    p.add_argument("--focal_gamma", default=0.0, type=_focal_gamma, help="focal loss (Lin et al. 2017): every sample's cross-entropy "
                   "term is scaled by (1 - the probability of its target) ** G inside the loss kernels, so easy samples count less; "
                   "finite and >= 0, 0 = off (the reference's behaviour); training, dev and test loss alike; composes with "
                   "--class_weights (the weights act as alpha), --label_smoothing, --aug_mixup / --aug_cutmix and --dp_exact")
    p.add_argument("--dp_overlap", action="store_true")
    p.add_argument("--dp_grad_comm", default="f32", choices=["f32", "bf16"], help="dtype of the gradient buckets on the links")
    p.add_argument("--dp_shard_optimizer", action="store_true",
                   help="per bucket: reduce-scatter of the gradients, AdamW on this rank's stripe, all-gather of the updated weights "
                        "(combines with --dp_overlap; the RCCL reduce-scatter / all-gather calls are rehearsed with gloo only so far)")
    p.add_argument("--dp_algorithm", default="all_reduce", choices=["all_reduce", "reduce_scatter_all_gather"],
                   help="gradient reduction per bucket: RCCL's all-reduce, or its two phases issued explicitly")
    p.add_argument("--dp_exact", action="store_true", help="data parallelism: BatchNorm statistics of the GLAC cells, the [B,B] similarity "
                   "matrices and the JS loss over the GLOBAL batch (the reference's single-GPU semantics) instead of per rank")
    p.add_argument("--cleanup_output", action="store_true", help="reference behaviour: rmtree('./output') at the end")
    p.add_argument("--data_path", default=None, type=str, help="directory with train.json, dev.json (or HFM's valid.json) and "
                   "test.json; without it the data is synthetic")
    p.add_argument("--img_path", default=None, type=str, help="directory of the <id>.jpg images (and inf.png) of --data_path")
    p.add_argument("--image_decode", default="host", choices=["host", "device"], help="with --data_path: decode the JPEG files in "
                   "the loader workers with Pillow (host), or only parse them there and decode them on the GPU, bit-identically "
                   "(device; files the device path does not take, e.g. progressive JPEGs, are still decoded on the host)")
    p.add_argument("--cache_dataset", default="off", choices=["off", "device"], help="with --data_path: decode and resize every "
                   "image once, keep the uint8 crops and the token tensors of every split in device memory (150,528 bytes per image "
                   "at 224 x 224) and build every batch there by index; the run takes the same steps as without it (d2r_amd.cache)")
    p.add_argument("--aug_crop_scale", default=1.0, type=_aug_crop_scale, help="with --data_path: random resized crop of the "
                   "training images on the device: a box of LO..1 of the image's area, aspect ratio 3/4..4/3, resized bilinearly to the "
                   "crop size (torchvision's RandomResizedCrop); in (0, 1], 1 = off, the reference's behaviour")
    p.add_argument("--aug_flip", default=0.0, type=_aug_flip, help="with --data_path: mirror each training image horizontally with "
                   "this probability, in [0, 1] (0 = off, the reference's behaviour); dev and test images are never augmented")
    for name, what in (("brightness", "brightness"), ("contrast", "contrast"), ("saturation", "saturation")):
        p.add_argument(f"--aug_{name}", default=0.0, type=_aug_jitter, help=f"with --data_path: scale the {what} of each training image "
                       "by a factor drawn uniformly from [max(0, 1 - J), 1 + J] (torchvision's ColorJitter; applied in the fixed order "
                       "brightness, contrast, saturation, hue); finite and >= 0, 0 = off; same rules as --aug_flip")
    p.add_argument("--aug_hue", default=0.0, type=_aug_hue, help="with --data_path: shift the hue of each training image by a fraction "
                   "of a turn drawn uniformly from [-H, H]; in [0, 0.5], 0 = off")
    p.add_argument("--aug_grayscale", default=0.0, type=_aug_flip, help="with --data_path: turn each training image grey with this "
                   "probability (torchvision's RandomGrayscale); in [0, 1], 0 = off")
    p.add_argument("--aug_erase", default=0.0, type=_aug_flip, help="with --data_path: with this probability, zero a random box of "
                   "2 %% to 33 %% of each normalised training image, aspect ratio 0.3 to 3.3 (torchvision's RandomErasing); in [0, 1], "
                   "0 = off")
    for name, what in (("delete", "delete it"), ("mask", "put [MASK] in its place"),
                       ("replace", "replace it by an id drawn uniformly from the vocabulary past its special and [unusedN] tokens")):
        p.add_argument(f"--aug_token_{name}", default=0.0, type=_aug_token, help="per token of a training text, with this "
                       f"probability: {what}, on the device (d2r_token_augment); [CLS] and [SEP] are kept, and a text keeps its "
                       "tokens if all would be deleted; in [0, 1], the three probabilities sum to at most 1, 0 = off, the reference's "
                       "behaviour; dev and test texts are never augmented; real and synthetic data")
    p.add_argument("--aug_whole_word", action="store_true", help="with --data_path: a word and its ## pieces share one --aug_token_* "
                   "decision, drawn at the word's first piece")
    p.add_argument("--aug_mixup", default=0.0, type=_aug_mix_alpha, help="MixUp of the training images on the device: each image is "
                   "blended with another image of its batch, lam * own + (1 - lam) * partner with lam ~ Beta(A, A) per sample, and the "
                   "loss is taken against both labels in these shares (d2r_image_mix, d2r_ce_mix_*); only the image is mixed, the text "
                   "stays the sample's own; finite and >= 0, 0 = off, the reference's behaviour; real and synthetic data")
    p.add_argument("--aug_cutmix", default=0.0, type=_aug_mix_alpha, help="CutMix of the training images on the device: a box of "
                   "1 - lam ~ Beta(A, A) of another image of the batch is pasted over each image, the label share corrected to the "
                   "clipped box (timm's rand_bbox); with --aug_mixup too, each sample takes CutMix with probability 0.5; same rules "
                   "as --aug_mixup")
    p.add_argument("--aug_mix_prob", default=None, type=_aug_mix_prob, help="probability that a training sample is mixed at all, in "
                   "[0, 1] (default 1); needs --aug_mixup or --aug_cutmix")
    p.add_argument("--pretrained", action="store_true", help="model configs, weights and image preprocessing from the local "
                   "--bert_name / --vit_name checkpoints (BertModel, CLIPModel.vision_model, preprocessor_config.json)")
    return p


def dataset_files(data_path: str):
    """(train, dev, test) JSON files of an MVSA / HFM directory: dev.json, or HFM's valid.json."""
    dev = os.path.join(data_path, "dev.json")
    if not os.path.exists(dev):
        dev = os.path.join(data_path, "valid.json")
    files = (os.path.join(data_path, "train.json"), dev, os.path.join(data_path, "test.json"))
    missing = [f for f in files if not os.path.exists(f)]
    if missing:
        raise SystemExit(f"--data_path {data_path}: missing {', '.join(missing)}")
    return files


def load_pretrained(args, weights: bool = True):
    """(text_config, vision_config, clip_vision_state_dict, bert_state_dict) from the local checkpoints (run.py:122-153);
    weights=False: the configs only (None, None for the state dicts)."""
    from transformers import BertConfig, BertModel, CLIPConfig, CLIPModel
    text_config = BertConfig.from_pretrained(args.bert_name)
    vision_config = CLIPConfig.from_pretrained(args.vit_name).vision_config
    if not weights:
        return text_config, vision_config, None, None
    clip_sd = CLIPModel.from_pretrained(args.vit_name).vision_model.state_dict()
    bert_sd = BertModel.from_pretrained(args.bert_name).state_dict()
    return text_config, vision_config, clip_sd, bert_sd


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.only_test and args.load_path is None:
        raise SystemExit("--only_test needs --load_path (the checkpoint to evaluate)")
    if (args.only_test or args.write_path is not None) and int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit("--only_test / --write_path run in a single process: start without torch.distributed.run (WORLD_SIZE 1)")
    if args.cache_dataset != "off" and args.data_path is None:
        raise SystemExit("--cache_dataset device caches the files of --data_path: synthetic data has nothing to decode; run without it")
    augment = args.aug_crop_scale < 1.0 or args.aug_flip > 0.0
    if augment and args.data_path is None:
        raise SystemExit("--aug_crop_scale / --aug_flip augment the uint8 crops of the images of --data_path: synthetic images are "
                         "not such crops; run without them")
    photo = {f[4:]: getattr(args, f) for f in PHOTO_FLAGS}
    photometric = any(v > 0.0 for v in photo.values())
    if photometric and args.data_path is None:
        raise SystemExit(f"{_PHOTO_NAMES} augment the uint8 crops of the images of --data_path: synthetic images are not such crops; "
                         "run without them")
    token_p = [getattr(args, f) for f in TOKEN_FLAGS]
    token_aug = any(v > 0.0 for v in token_p)
    if sum(token_p) > 1.0:
        raise SystemExit(f"{_TOKEN_NAMES} are the probabilities of one choice per token: their sum {sum(token_p):g} must be <= 1")
    if args.aug_whole_word and args.data_path is None:
        raise SystemExit("--aug_whole_word reads the word pieces from the vocabulary of --bert_name: synthetic ids are plain integers "
                         "without one; run without it")
    mixing = args.aug_mixup > 0.0 or args.aug_cutmix > 0.0
    if args.aug_mix_prob is not None and not mixing:
        raise SystemExit("--aug_mix_prob is the probability of --aug_mixup / --aug_cutmix: give one of them too")
    try:
        class_weights = parse_class_weights(args.class_weights, args.num_classes)
    except ValueError as e:
        raise SystemExit(str(e))
    if class_weights is not None and args.dp_exact:
        # each rank divides by the weight sum of ITS labels (as DDP around the reference's loss would): with class weights that is
        # not the global-batch loss --dp_exact promises
        raise SystemExit("--dp_exact reproduces the global-batch loss, which per-rank class-weight normalisation does not: "
                         "use --class_weights none with --dp_exact (--label_smoothing is fine)")
    from .config import TextConfig, VisionConfig
    from .data import MSDDataset, SyntheticMSDDataset, make_loader
    from .image import CLIP_MEAN, CLIP_STD, RESCALE, ClipCollate, processor_settings
    from .dp import init_process_group_from_env
    from .modules import UnimoModelF
    from .train import MSDTrainer

    rank, world = init_process_group_from_env()
    if args.device == "cuda":
        args.device = f"cuda:{int(os.environ.get('LOCAL_RANK', '0'))}"
    args.compute_dtype = {"bf16": torch.bfloat16, "fp16": torch.float16, "f32": torch.float32}[args.dtype]
    set_seed(args.seed)
    if args.save_path is not None and rank == 0:
        os.makedirs(args.save_path, exist_ok=True)
    logger.info(args)
    if args.batch_size % world:
        raise SystemExit(f"--batch_size {args.batch_size} must be divisible by the world size {world}")
    per_rank = args.batch_size // world
    clip_sd = bert_sd = None
    if args.pretrained:
        # --only_test: configs and preprocessing from the local directories, every weight from the checkpoint
        text_config, vision_config, clip_sd, bert_sd = load_pretrained(args, weights=not args.only_test)
        R, S, mean, std, rescale = processor_settings(args.vit_name)
        if S != vision_config.image_size:
            raise SystemExit(f"{args.vit_name}: the processor crops {S} x {S} but the vision model takes {vision_config.image_size}")
        args.image_size, args.patch_size = vision_config.image_size, vision_config.patch_size
    else:
        text_config = TextConfig(num_hidden_layers=args.encoder_layers, hidden_dropout_prob=args.bert_dropout,
                                 attention_probs_dropout_prob=args.bert_dropout)
        vision_config = VisionConfig(num_hidden_layers=args.encoder_layers, image_size=args.image_size, patch_size=args.patch_size)
        R, S, mean, std, rescale = args.image_size, args.image_size, CLIP_MEAN, CLIP_STD, RESCALE
    ntok = (args.image_size // args.patch_size) ** 2 + 1
    if args.data_path is not None:
        if args.img_path is None:
            raise SystemExit("--data_path needs --img_path")
        files = dataset_files(args.data_path)
        collate = ClipCollate(R, S, mean, std, rescale, image_decode=args.image_decode)

    def loader(n, seed, shuffle, split):
        if args.data_path is None:
            ds = SyntheticMSDDataset(n, args.max_seq, args.image_size, args.num_classes, seed=seed, num_image_tokens=ntok)
        else:
            ds = MSDDataset(files[split], args.img_path, args.bert_name, args.max_seq, image_decode=args.image_decode,
                            labels_optional=args.only_test and split == 2)  # unlabelled posts: only the test split of --only_test
        sampler = None
        if world > 1 and shuffle:  # only the TRAINING set is sharded; every rank evaluates the whole dev / test set
            sampler = torch.utils.data.distributed.DistributedSampler(ds, num_replicas=world, rank=rank, shuffle=shuffle,
                                                                      seed=args.seed)
        return make_loader(ds, per_rank, shuffle, args.num_workers, drop_last=shuffle, sampler=sampler,
                           collate_fn=None if args.data_path is None else collate)

    if not args.only_test:
        train_dl, dev_dl = loader(args.train_samples, 1, True, 0), loader(args.eval_samples, 2, False, 1)
    test_dl = loader(args.eval_samples, 3, False, 2)
    augmenter = None
    if augment and args.only_test:
        logger.info("--aug_crop_scale / --aug_flip are ignored with --only_test: only training batches are augmented")
    if photometric and args.only_test:
        logger.info("%s are ignored with --only_test: only training batches are augmented", _PHOTO_NAMES)
    elif photometric and float(rescale) != RESCALE:
        raise SystemExit(f"{_PHOTO_NAMES} work on pixel values in [0, 1] and need the preprocessor's rescale_factor to be 1/255, "
                         f"got rescale_factor = {rescale!r}")
    if (augment or photometric) and not args.only_test:
        # generators of its own, seeded from (--seed, rank): each rank augments its shard with its own streams, and the default
        # generator (samplers, dropout seeds) is never drawn from; the photometric options alone leave the boxes the identity
        from .augment import Augmenter
        if photometric:
            augmenter = Augmenter(S, args.aug_crop_scale, args.aug_flip, seed=args.seed, rank=rank, brightness=photo["brightness"],
                                  contrast=photo["contrast"], saturation=photo["saturation"], hue=photo["hue"],
                                  grayscale_p=photo["grayscale"], erase_p=photo["erase"], norm=(mean, std, rescale))
        else:
            augmenter = Augmenter(S, args.aug_crop_scale, args.aug_flip, seed=args.seed, rank=rank)
    text_augmenter = None
    if (token_aug or args.aug_whole_word) and args.only_test:
        logger.info("%s / --aug_whole_word are ignored with --only_test: only training batches are augmented", _TOKEN_NAMES)
    elif token_aug:
        # a generator of its own, seeded from (--seed, rank), as the image augmenter's
        from .text_augment import TokenAugmenter
        if args.data_path is None:
            settings = dict(SYNTHETIC_TOKENS, vocab=int(text_config.vocab_size))
        else:
            settings = token_settings(train_dl.dataset.tokenizer, args.aug_whole_word, args.aug_token_mask > 0.0)
        try:
            text_augmenter = TokenAugmenter(*token_p, seed=args.seed, rank=rank, **settings)
        except ValueError as e:
            raise SystemExit(f"{_TOKEN_NAMES}: {e}")
    elif args.aug_whole_word:
        logger.info("--aug_whole_word has no effect without %s", _TOKEN_NAMES)
    mixer = None
    if mixing and args.only_test:
        logger.info("--aug_mixup / --aug_cutmix / --aug_mix_prob are ignored with --only_test: only training batches are mixed")
    elif mixing:
        # a generator of its own, seeded from (--seed, rank), as the augmenters'; the trainer holds it with and without the cache
        from .mix import Mixer
        mixer = Mixer(int(S), args.aug_mixup, args.aug_cutmix, 1.0 if args.aug_mix_prob is None else args.aug_mix_prob, seed=args.seed,
                      rank=rank)
    if args.cache_dataset == "device" and args.only_test:
        logger.info("--cache_dataset device is ignored with --only_test: a single pass over the test split gains nothing")
    elif args.cache_dataset == "device":
        # every rank caches the whole of each split (the training shards change every epoch); the default generator is untouched
        from .cache import cache_loaders
        more = {} if text_augmenter is None else {"text_augmenters": {"train": text_augmenter}}
        cached = cache_loaders({"train": train_dl, "dev": dev_dl, "test": test_dl}, args.device, logger,
                               augmenters={"train": augmenter} if augmenter is not None else None, **more)
        train_dl, dev_dl, test_dl = cached["train"], cached["dev"], cached["test"]
        augmenter = text_augmenter = None  # the cached training loader augments its own batches
    if args.ema_decay and args.only_test:
        logger.info("--ema_decay is ignored with --only_test: the checkpoint already holds the weights that were saved")
        args.ema_decay = 0.0
    if args.only_test and (args.layer_lr_decay != 1.0 or args.wd_exempt_1d or args.weight_decay != 1e-2):
        logger.info("--layer_lr_decay / --wd_exempt_1d / --weight_decay are ignored with --only_test: no optimiser step is taken")
        args.layer_lr_decay, args.wd_exempt_1d, args.weight_decay = 1.0, False, 1e-2
    if args.only_test and args.drop_path:
        logger.info("--drop_path is ignored with --only_test: stochastic depth acts on training steps only")
        args.drop_path = 0.0
    if args.only_test and args.patch_dropout:
        logger.info("--patch_dropout is ignored with --only_test: patches are dropped in training steps only")
        args.patch_dropout = 0.0
    if class_weights == "balanced":
        try:
            class_weights = balanced_class_weights(train_label_counts(args, None if args.data_path is None else files[0]))
        except ValueError as e:
            raise SystemExit(str(e))
    args.class_weights = class_weights  # what the model reads: a list of num_classes floats, or None
    if class_weights is not None or args.label_smoothing or args.focal_gamma:
        logger.info("cross entropy: class weights %s, label smoothing %g, focal gamma %g%s", class_weights, args.label_smoothing,
                    args.focal_gamma, " (no loss is computed with --only_test: no effect)" if args.only_test else "")
    model = UnimoModelF(args=args, vision_config=vision_config, text_config=text_config, num_classes=args.num_classes)
    if args.only_test:
        trainer = MSDTrainer(test_data=test_dl, model=model, args=args, logger=logger, writer=None)
        trainer._load_checkpoint(args.load_path)  # strict: every key of the model, nothing else
        trainer.predict(test_dl, args.write_path)
        return
    more = {} if text_augmenter is None else {"text_augmenter": text_augmenter}
    if mixer is not None:
        more["mixer"] = mixer
    trainer = MSDTrainer(train_data=train_dl, dev_data=dev_dl, test_data=test_dl, model=model, args=args, logger=logger,
                         writer=None, augmenter=augmenter, **more)
    trainer.train(clip_sd, bert_sd)  # None, None without --pretrained: randomly initialised encoders
    if trainer.samples_per_sec:
        logger.info("training throughput: %.1f samples/s on %d GPU(s)", trainer.samples_per_sec, world)
    if args.write_path is not None:  # with the weights test() ran on: the best checkpoint when the run saved one
        with contextlib.nullcontext() if args.load_path is not None else trainer.optimizer.ema_weights():
            trainer.predict(test_dl, args.write_path)


if __name__ == "__main__":
    main()
