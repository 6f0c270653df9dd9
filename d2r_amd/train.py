"""MSDTrainer — drop-in counterpart of the reference's training loop (modules/train.py:53-328) on the HIP path.

Same constructor, same public methods (``train(clip_model_dict, bert_model_dict)``, ``evaluate(epoch)``,
``test(epoch)``, ``_step(batch, mode)``), same weight-ingest rename rule and coverage assert (:92-111), same
optimiser grouping / learning rates / schedule (:287-328), same best-dev-F1 checkpoint with the reference's
state-dict key names (:210-216).  Differences, all deliberate:
  * AdamW and the schedule are the fused HIP kernel over flat buffers (d2r_amd.params);
  * the per-step host sync ``loss.item()`` (:123) is replaced by an on-device running sum read every
    ``refresh_step`` steps;
  * ``shutil.rmtree("./output")`` (:149) is opt-in (``args.cleanup_output``);
  * optional data parallelism (args.world_size > 1 via torch.distributed, see d2r_amd.dp);
  * optional extensions: gradient clipping (args.max_grad_norm) and a weight EMA (args.ema_decay: evaluate() / test() run on
    the averaged weights and best_model.pth holds them; BatchNorm running statistics stay the live ones), layer-wise lr decay and
    no weight decay on 1-D parameters (args.layer_lr_decay, args.wd_exempt_1d), the weight decay itself (args.weight_decay),
    stochastic depth of the two encoder towers in training steps (args.drop_path; its seeds come from a generator of its own),
    PatchDropout of the vision tower in training steps (args.patch_dropout, d2r_amd.patch_dropout: a sampler with a generator of
    its own on the vision embedding; evaluate() / test() / predict() see all patches);
  * optional image augmentation of the TRAINING batches (``augmenter``, d2r_amd.augment: random resized crop and flip, colour
    jitter, random grayscale and random erasing on the device; a CachedLoader carries its own); evaluate() / test() / predict()
    never augment;
  * optional text augmentation of the TRAINING batches (``text_augmenter``, d2r_amd.text_augment: token deletion, [MASK] and
    random-id replacement in one launch on the device; a CachedLoader carries its own), under the same rules;
  * optional MixUp / CutMix of the TRAINING batches (``mixer``, d2r_amd.mix: one launch on the finished pixel batch, after every
    other augmentation and the same for cached and uncached loaders; the loss takes two labels per sample), under the same rules;
  * evaluate() / test() count a confusion matrix on the device (d2r_confusion_add) instead of copying labels and predictions to
    the host per batch, and log per-class precision / recall / F1 / support after the four aggregates; they return the scalar
    entries as before, the whole result (with "confusion" and "per_class") stays in last_dev_result / last_test_result.
"""
from __future__ import annotations

import json
import logging
import os
import shutil
import time
from typing import Optional

import torch

from . import functional as F
from .dp import DataParallel
from .jpeg import DecodeLog
from .params import FusedAdamW, LinearWarmupSchedule, ParamStore


def get_four_metrics(labels, predicted_labels, type="weighted"):
    """(accuracy, recall, precision, F1) with sklearn's class-support weighting — the tuple order the reference's
    loops unpack (modules/train.py:23-30, used at :195 and :255)."""
    from sklearn.metrics import accuracy_score, precision_recall_fscore_support
    precision, recall, f1, _ = precision_recall_fscore_support(labels, predicted_labels, average=type, zero_division="warn")
    return accuracy_score(labels, predicted_labels), recall, precision, f1


def metrics_from_confusion(cm):
    """The four numbers of get_four_metrics plus the per-class view, from a confusion matrix alone (cm[label][prediction], integer
    counts: a nested list, numpy array or host tensor): {"eval_accuracy", "precision", "recall", "f_score", "per_class": [{"class",
    "precision", "recall", "f1", "support"} per class], "confusion": nested list}.  float64 with sklearn's operations in sklearn's
    order (precision_recall_fscore_support(average="weighted", zero_division -> 0): per-class tp / predicted, tp / true and
    2 tp / (true + predicted) with 0 for an empty denominator, np.average(x, weights=support) over the classes that occur among
    the labels or the predictions; accuracy_score: trace / total), so the aggregates are bit-identical to get_four_metrics on the
    labels and predictions the matrix was counted from."""
    import numpy as np
    cm = np.asarray(cm, dtype=np.int64)
    if cm.ndim != 2 or cm.shape[0] != cm.shape[1] or cm.shape[0] < 1 or (cm < 0).any():
        raise ValueError(f"metrics_from_confusion: a square matrix of non-negative counts is expected, got shape {cm.shape}")
    total = int(cm.sum())
    if total == 0:
        raise ValueError("metrics_from_confusion: the matrix counts no sample")
    tp, true_sum, pred_sum = np.diag(cm), cm.sum(axis=1), cm.sum(axis=0)

    def divide(num, den):  # sklearn's _prf_divide with zero_division -> 0
        den = den.astype(np.float64)
        empty = den == 0
        den[empty] = 1
        out = num.astype(np.float64) / den
        out[empty] = 0.0
        return out

    precision, recall = divide(tp, pred_sum), divide(tp, true_sum)
    f1 = divide((1 + 1.0) * tp.astype(np.float64), 1.0 * true_sum.astype(np.float64) + pred_sum.astype(np.float64))
    seen = (true_sum + pred_sum) > 0  # sklearn's label set: the classes among the labels or the predictions
    avg = lambda x: float(np.average(x[seen], weights=true_sum[seen]))
    return {"eval_accuracy": float(np.float64(int(tp.sum())) / np.float64(total)), "precision": avg(precision), "recall": avg(recall),
            "f_score": avg(f1),
            "per_class": [{"class": c, "precision": float(precision[c]), "recall": float(recall[c]), "f1": float(f1[c]),
                           "support": int(true_sum[c])} for c in range(cm.shape[0])],
            "confusion": cm.tolist()}


def log_per_class(logger, metrics):
    """The confusion matrix and one line per class, after the aggregate lines of evaluate() / test() / predict() (which stay as
    they were: one "  key = value" line per scalar)."""
    logger.info("  confusion matrix (row: label, column: prediction): %s", metrics["confusion"])
    for pc in metrics["per_class"]:
        logger.info("  class %d: precision %.6f, recall %.6f, f1 %.6f, support %d", pc["class"], pc["precision"], pc["recall"],
                    pc["f1"], pc["support"])


def _reference_keys(result):
    """What evaluate() / test() return: the scalar entries the reference's loops produce.  The confusion matrix and the per-class
    view stay in MSDTrainer.last_dev_result / last_test_result (the whole dict, as logged)."""
    return {k: v for k, v in result.items() if k not in ("confusion", "per_class")}


def write_predictions(path, ids, labels, preds, probs, paths_text, paths_image):
    """JSON Lines, one object per sample in dataset order: {"index", "id", "label", "pred", "probs", "paths_text", "paths_image"}.
    ids / labels: host lists (None where unknown); preds: int64 [N]; probs, paths_*: fp32 [N, *] host tensors.  Every float is the
    fp32 value as a Python float, so it reads back exactly."""
    preds, probs, pt, pi = preds.tolist(), probs.tolist(), paths_text.tolist(), paths_image.tolist()
    with open(path, "w", encoding="utf-8") as f:
        for i in range(len(preds)):
            f.write(json.dumps({"index": i, "id": ids[i], "label": labels[i], "pred": preds[i], "probs": probs[i],
                                "paths_text": pt[i], "paths_image": pi[i]}) + "\n")


def _pretrained_source(name: str):
    """Where a model key comes from: ('clip' | 'bert' | None, key inside that checkpoint).  The reference's rule
    (modules/train.py:95-107): a key containing 'vision' is looked up in the CLIP-ViT state dict with every 'vision_' and
    'model.' removed; otherwise a key containing 'text' is looked up in the BERT state dict with 'text_' and 'model.' removed."""
    for marker, source in (("vision", "clip"), ("text", "bert")):
        if marker in name:
            return source, name.replace(marker + "_", "").replace("model.", "")
    return None, None


def ingest_pretrained(model, clip_model_dict, bert_model_dict):
    """Copies pretrained CLIP-ViT / BERT tensors into the model by the rename rule above and insists, like the reference
    (modules/train.py:109-110), that EVERY key of both checkpoints found a destination."""
    merged = model.state_dict()
    sources = {"clip": clip_model_dict, "bert": bert_model_dict}
    used = {"clip": set(), "bert": set()}
    for name in list(merged):
        source, key = _pretrained_source(name)
        if source is not None and key in sources[source]:
            merged[name] = sources[source][key]
            used[source].add(key)
    for source, ckpt in sources.items():
        missing = [k for k in ckpt if k not in used[source]]
        assert not missing, f"{len(missing)} pretrained {source} tensors have no destination in the model, e.g. {missing[:5]}"
    model.load_state_dict(merged)


class MSDTrainer:
    def __init__(self, train_data=None, dev_data=None, test_data=None, model=None, args=None, logger=None,
                 writer=None, augmenter=None, *, text_augmenter=None, mixer=None) -> None:
        self.train_data, self.dev_data, self.test_data = train_data, dev_data, test_data
        self.mixer = mixer  # MixUp / CutMix of the training batches (d2r_amd.mix), after every other augmentation; None: off
        self.augmenter = augmenter  # training batches of packed images only (a CachedLoader augments its own batches)
        self.text_augmenter = text_augmenter  # training batches' token tensors (a CachedLoader with its own: None here)
        self.model, self.args = model, args
        self.logger = logger or logging.getLogger(__name__)
        self.writer = writer
        self.step = 0
        self.refresh_step = 2
        self.decode_log = DecodeLog(self.logger)  # --image_decode device: device / host split and decode status per epoch
        self.best_dev_metric = 0
        self.best_dev_epoch = None
        self.optimizer = None
        self.samples_per_sec = None
        self.last_dev_result = self.last_test_result = None  # the last evaluate() / test() pass: its result with "confusion" and "per_class"
        if self.train_data is not None:
            self.train_num_steps = len(self.train_data) * args.num_epochs
        self.multiModal_before_train()

    # -- optimiser / schedule (modules/train.py:287-328) ----------------------------------------------
    def multiModal_before_train(self):
        dtype = getattr(self.args, "compute_dtype", torch.float32)
        self.model.to(self.args.device)
        self.model.set_compute_dtype(dtype)
        self.store = ParamStore(self.model, dtype)
        from . import configure_runtime
        configure_runtime()
        self.optimizer = FusedAdamW(self.store, lr=self.args.lr, fc_lr=5e-2, weight_decay=float(getattr(self.args, "weight_decay", 1e-2)),
                                    max_grad_norm=getattr(self.args, "max_grad_norm", None) or None,
                                    ema_decay=getattr(self.args, "ema_decay", None) or None,
                                    layer_lr_decay=getattr(self.args, "layer_lr_decay", None) or None,
                                    decay_exempt_1d=bool(getattr(self.args, "wd_exempt_1d", False)))
        if dtype == torch.float16:  # fp16 activation gradients need a scaled loss (AMP's GradScaler, here inside the optimiser)
            self.optimizer.enable_loss_scaling()
        shard = bool(getattr(self.args, "dp_shard_optimizer", False))
        self.dp = DataParallel(self.store, self.optimizer, self.model,
                               overlap=bool(getattr(self.args, "dp_overlap", False)),
                               grad_comm_dtype=torch.bfloat16 if getattr(self.args, "dp_grad_comm", "f32") == "bf16" else torch.float32,
                               shard_optimizer=shard, algorithm=getattr(self.args, "dp_algorithm", "all_reduce"),
                               global_batch_exact=bool(getattr(self.args, "dp_exact", False)))
        self.dp.broadcast_parameters()
        # stochastic depth: per-layer rates on the two towers, and DropPath's own generator seeded from (seed, rank) - the default
        # generator is not drawn from.  Off (0) leaves the model as it was built.
        self.drop_path_rates = None
        rate = float(getattr(self.args, "drop_path", 0.0) or 0.0)
        if rate > 0.0 and self.train_data is not None:
            self.drop_path_rates = self.model.model.set_drop_path(rate)
            F.seed_drop_path(int(getattr(self.args, "seed", 0)), self.dp.rank)
        # PatchDropout: a sampler on the vision embedding with a generator of its own, seeded from (seed, rank); K depends on the
        # flag and the patch grid alone, so it is the same on every rank.  Off (0) builds no generator and leaves the model as it was.
        self.patch_dropout = None
        rate = float(getattr(self.args, "patch_dropout", 0.0) or 0.0)
        if rate > 0.0 and self.train_data is not None:
            self.patch_dropout = self.model.model.set_patch_dropout(rate, int(getattr(self.args, "seed", 0)), self.dp.rank)
        if self.train_data is not None:
            self.scheduler = LinearWarmupSchedule(self.optimizer, self.args.warmup_ratio * self.train_num_steps,
                                                  self.train_num_steps)

    def _load_checkpoint(self, path):
        self.logger.info("Loading model from {}".format(path))
        self.model.load_state_dict(torch.load(path, map_location=self.args.device))
        self.store.refresh_lowp()
        self.logger.info("Load model successful!")

    def _to_device(self, batch, augmenter=None, text_augmenter=None):
        # tensors are copied; a packed batch of images (MSDDataset + ClipCollate: PackedImages, or PackedJpegImages with
        # image_decode="device") becomes its CLIP pixel values on the device - through `augmenter` when the training loop passes one;
        # the three token tensors go through `text_augmenter` once they are there, when the training loop passes one
        def pixel_values(t):
            return t.to_pixel_values(self.args.device) if augmenter is None else augmenter.apply_packed(t, self.args.device)
        moved = tuple(t.to(self.args.device, non_blocking=True) if isinstance(t, torch.Tensor) else
                      pixel_values(t) if hasattr(t, "to_pixel_values") else t for t in batch)
        if text_augmenter is None:
            return moved
        return (*text_augmenter.apply_batch(*moved[:3]), *moved[3:])

    # -- training (modules/train.py:77-159) -----------------------------------------------------------
    def train(self, clip_model_dict=None, bert_model_dict=None):
        self.step = 0
        self.model.train()
        self.logger.info("***** Running training *****")
        self.logger.info("  Num instance = %d", len(self.train_data) * self.args.batch_size)
        self.logger.info("  Num epoch = %d", self.args.num_epochs)
        self.logger.info("  Batch size = %d", self.args.batch_size)
        self.logger.info("  Learning rate = {}".format(self.args.lr))
        self.logger.info("  Evaluate begin = %d", self.args.eval_begin_epoch)
        if self.args.load_path is not None:
            self._load_checkpoint(self.args.load_path)
        if clip_model_dict is not None and bert_model_dict is not None:
            ingest_pretrained(self.model, clip_model_dict, bert_model_dict)
            self.store.refresh_lowp()
        if self.optimizer.ema is not None:  # the average starts from the weights training starts from
            self.optimizer.ema_reset()
            self.logger.info("  Weight EMA: decay %g with warm-up min(decay, (1 + t) / (10 + t)); %d bytes of device memory "
                             "(4 per live parameter); evaluation and best_model.pth use the averaged weights",
                             self.optimizer.ema_decay, 4 * self.store.n)
        if self.optimizer.table is not None:
            self.logger.info("  AdamW hyper-parameters per parameter: %d segments in one launch (layer_lr_decay %s, weight decay %g%s); "
                             "smallest lr scale: text tower %g, vision tower %g", len(self.optimizer.table),
                             self.optimizer.layer_lr_decay, self.optimizer.param_groups[0]["weight_decay"],
                             ", none on 1-D parameters" if self.optimizer.decay_exempt_1d else "", *self.optimizer.tower_lr_scales)
        if self.drop_path_rates is not None:
            self.logger.info("  Stochastic depth (training steps only): drop_path per layer, text tower [%s], vision tower [%s]",
                             *(", ".join(f"{r:.4g}" for r in rs) for rs in self.drop_path_rates))
        if self.patch_dropout is not None:
            self.logger.info("  PatchDropout (training steps only): %s", self.patch_dropout.describe())
        augmenter = self.augmenter or getattr(self.train_data, "augmenter", None)
        if augmenter is not None:
            self.logger.info("  Image augmentation of the training batches: %s", augmenter.describe())
        text_augmenter = self.text_augmenter or getattr(self.train_data, "text_augmenter", None)
        if text_augmenter is not None:
            self.logger.info("  Text augmentation of the training batches: %s", text_augmenter.describe())
        if self.mixer is not None:
            self.logger.info("  MixUp / CutMix of the training batches: %s", self.mixer.describe())
        run_loss = torch.zeros((), dtype=torch.float32, device=self.args.device)
        clipping = self.optimizer.max_grad_norm is not None
        grad_norm = torch.zeros((), dtype=torch.float32, pin_memory=torch.cuda.is_available()) if clipping else None
        # throughput of the TRAINING loop only: the clock starts after a few warm-up steps (first-touch allocations,
        # loader workers) and stops across evaluation
        t_train, t_mark, seen, warm = 0.0, None, 0, 5
        epoch = 0
        for epoch in range(1, self.args.num_epochs + 1):
            sampler = getattr(self.train_data, "sampler", None)
            if hasattr(sampler, "set_epoch"):  # DistributedSampler: a new shuffle every epoch
                sampler.set_epoch(epoch)
            if self.step >= warm:
                t_mark = time.time()
            for batch in self.train_data:
                self.step += 1
                if self.step == warm + 1 and t_mark is None:
                    t_mark = time.time()
                packed, batch = batch, self._to_device(batch, self.augmenter, self.text_augmenter)
                if self.mixer is not None:  # after every other augmentation, cached loader or not: the images and the labels only
                    images, labels, labels_b, lam = self.mixer.apply(batch[5], batch[4])
                    batch = (*batch[:4], labels, images, labels_b, lam)
                self.decode_log.note(packed)
                self.dp.begin_step()
                (loss, logits), labels = self._step(batch, mode="train")
                F._lib.call("d2r_axpby", F.F32, 1.0, loss.detach().data_ptr(), 1.0, run_loss.data_ptr(), 1, F._stream())
                self.optimizer.backward(loss)
                self.dp.reduce_gradients()
                self.optimizer.step()
                self.dp.gather_parameters()  # (sharded optimiser only: publish this rank's slice of the updated weights)
                self.scheduler.step()
                self.optimizer.zero_grad()
                if self.step > warm:
                    seen += int(labels.shape[0]) * self.dp.world
                if self.step % self.refresh_step == 0:
                    if clipping:  # the pre-clip norm of this step: lands with the sync below, no wait of its own
                        grad_norm.copy_(self.optimizer.last_grad_norm, non_blocking=True)
                    avg_loss = float(run_loss.item()) / self.refresh_step  # the only host sync of the loop
                    run_loss.zero_()
                    self.decode_log.poll()  # decode status of the batches so far: complete after the sync above
                    if t_mark is not None and seen:
                        self.samples_per_sec = seen / max(t_train + time.time() - t_mark, 1e-9)
                    if clipping:
                        self.logger.info("step %d loss:%-6.5f samples/s:%.1f grad_norm:%.4f", self.step, avg_loss,
                                         self.samples_per_sec or 0.0, float(grad_norm))
                    else:
                        self.logger.info("step %d loss:%-6.5f samples/s:%.1f", self.step, avg_loss, self.samples_per_sec or 0.0)
                    if self.writer:
                        self.writer.add_scalar(tag="train_loss", scalar_value=avg_loss, global_step=self.step)
            self.decode_log.end_epoch(epoch)
            if t_mark is not None:
                if self.args.device != "cpu" and torch.cuda.is_available():
                    torch.cuda.synchronize()
                t_train += time.time() - t_mark
                t_mark = None
            if epoch >= self.args.eval_begin_epoch and self.dev_data is not None:
                self.evaluate(epoch)
        if seen and t_train > 0:
            self.samples_per_sec = seen / t_train
        if self.test_data is not None:
            if self.args.save_path is not None and os.path.exists(self.args.save_path + "best_model.pth"):
                self.args.load_path = self.args.save_path + "best_model.pth"
            self.test(epoch)
        if getattr(self.args, "cleanup_output", False) and os.path.isdir("./output"):
            shutil.rmtree("./output")  # the reference does this unconditionally (modules/train.py:149)

    def _eval_loop(self, data, desc):
        """One pass over `data`: the loss sum and the confusion matrix (d2r_confusion_add: argmax and counting in one launch per batch)
        stay on the device, nothing is copied to the host per batch; one copy at the end, the metrics on the host from the exact
        integer matrix (metrics_from_confusion)."""
        classes = self.model.fc.weight.shape[0]
        # [C * C counts | the fp32 loss sum in the low half of one more int64]: one allocation, one copy to the host
        acc = torch.zeros(classes * classes + 1, dtype=torch.int64, device=self.args.device)
        counts, total_loss = acc[:classes * classes].view(classes, classes), acc[classes * classes:].view(torch.float32)[:1]
        with torch.no_grad():
            for batch in data:
                batch = self._to_device(batch)
                (loss, logits), labels = self._step(batch, mode=desc)
                F._lib.call("d2r_axpby", F.F32, 1.0, loss.data_ptr(), 1.0, total_loss.data_ptr(), 1, F._stream())
                F.confusion_add(logits, labels.view(-1).long(), counts)  # (.long(): the same tensor when it is int64 already)
        host = acc.cpu()  # the only host sync of the pass
        result = metrics_from_confusion(host[:classes * classes].view(classes, classes).numpy())
        result["loss"] = float(host[classes * classes:].view(torch.float32)[0])
        return result

    def evaluate(self, epoch):
        # Data parallel: every rank evaluates the WHOLE dev set (the loaders of d2r_amd.run shard only the training set), on
        # identical weights and — after the line below — identical BatchNorm running statistics, so every rank takes the
        # same best-model decision and rank 0's checkpoint is the model all ranks hold.
        self.dp.sync_buffers()
        self.model.eval()
        self.logger.info("***** Running evaluate *****")
        self.logger.info("  Num instance = %d", len(self.dev_data) * self.args.batch_size)
        self.logger.info("  Batch size = %d", self.args.batch_size)
        with self.optimizer.ema_weights():  # --ema_decay: the averaged weights, also in the checkpoint; a no-op without
            result = self._eval_loop(self.dev_data, "dev")
            result["global_step"] = epoch
            self.logger.info("***** Dev Eval results *****")
            for key in sorted(result.keys()):
                if key not in ("confusion", "per_class"):
                    self.logger.info("  %s = %s", key, str(result[key]))
            log_per_class(self.logger, result)
            f1, acc = result["f_score"], result["eval_accuracy"]
            if self.writer:
                self.writer.add_scalar(tag="dev_acc", scalar_value=acc, global_step=epoch)
                self.writer.add_scalar(tag="dev_f1", scalar_value=f1, global_step=epoch)
                self.writer.add_scalar(tag="dev_loss", scalar_value=result["loss"] / len(self.dev_data), global_step=epoch)
            self.logger.info("Epoch {}/{}, best dev f1: {}, best epoch: {}, current dev f1 score: {}, acc: {}.".format(
                epoch, self.args.num_epochs, self.best_dev_metric, self.best_dev_epoch, f1, acc))
            if f1 >= self.best_dev_metric:
                self.logger.info("Get better performance at epoch {}".format(epoch))
                self.best_dev_epoch = epoch
                self.best_dev_metric = f1
                if self.args.save_path is not None and self.dp.rank == 0:
                    os.makedirs(self.args.save_path, exist_ok=True)
                    torch.save(self.model.state_dict(), self.args.save_path + "best_model.pth")
                    self.logger.info("Save best model at {}".format(self.args.save_path))
        # unconditional: every rank reaches it whatever it decided above (a collective behind a per-rank floating-point
        # comparison could pair with the next one); nobody looks for / loads best_model.pth while rank 0 is still writing it
        self.dp.barrier()
        self.model.train()
        self.last_dev_result = result
        return _reference_keys(result)

    def test(self, epoch):
        self.model.eval()
        self.logger.info("\n***** Running testing *****")
        self.logger.info("  Num instance = %d", len(self.test_data) * self.args.batch_size)
        self.logger.info("  Batch size = %d", self.args.batch_size)
        if self.args.load_path is not None:  # (with --ema_decay the checkpoint holds the averaged weights already)
            self._load_checkpoint(self.args.load_path)
            result = self._eval_loop(self.test_data, "test")
        else:
            with self.optimizer.ema_weights():
                result = self._eval_loop(self.test_data, "test")
        result["global_step"] = epoch
        self.logger.info("***** Test Eval results *****")
        for key in sorted(result.keys()):
            if key not in ("confusion", "per_class"):
                self.logger.info("  %s = %s", key, str(result[key]))
        log_per_class(self.logger, result)
        if self.writer:
            self.writer.add_scalar(tag="test_acc", scalar_value=result["eval_accuracy"])
            self.writer.add_scalar(tag="test_f1", scalar_value=result["f_score"])
            self.writer.add_scalar(tag="test_loss", scalar_value=result["loss"] / len(self.test_data))
        self.model.train()
        self.last_test_result = result
        return _reference_keys(result)

    def predict(self, data, write_path=None):
        """Label-free prediction over `data` (eval mode, no_grad): logits, class probabilities (d2r_softmax_fwd), predicted class
        (d2r_argmax_rows) and the per-sample router outputs of both routing modules stay on the device across batches and are
        copied to the host once at the end.  Metrics (test()'s four, "confusion" and "per_class": metrics_from_confusion on the matrix
        of the labels and predictions held here) when every sample is labelled (label >= 0); JSON Lines
        records (write_predictions) with `write_path`.  -> dict of host tensors / lists, "metrics" (or None), "samples_per_sec"."""
        self.model.eval()
        self.logger.info("***** Running prediction *****")
        self.logger.info("  Num instance = %d", len(data.dataset))
        self.logger.info("  Batch size = %d", data.batch_size)
        ds = data.dataset
        in_order = isinstance(data.sampler, torch.utils.data.SequentialSampler)
        logits_l, probs_l, preds_l, pt_l, pi_l, labels_l = [], [], [], [], [], []
        t0 = time.time()
        with torch.no_grad():
            for packed in data:
                input_ids, input_mask, segment_ids, _, _, images = self._to_device(packed)
                self.decode_log.note(packed)  # after _to_device: a device-decoded batch has its status tensor from then on
                _, logits = self.model(input_ids=input_ids, attention_mask=input_mask, token_type_ids=segment_ids, labels=None,
                                       images=images)
                aux = self.model.last_aux
                logits_l.append(logits)
                probs_l.append(F.softmax_rows(logits))
                preds_l.append(F.argmax_rows(logits))
                pt_l.append(aux["paths_text"])
                pi_l.append(aux["paths_image"])
                labels_l.append(packed[4])  # the loader's host copy: no device round trip
        if not logits_l:
            raise ValueError("predict: the loader yielded no batch")
        dev = [torch.cat(x) for x in (logits_l, probs_l, preds_l, pt_l, pi_l)]
        logits, probs, preds, paths_text, paths_image = [t.cpu() for t in dev]  # the one copy to the host
        n = int(preds.shape[0])
        self.samples_per_sec = n / max(time.time() - t0, 1e-9)
        self.decode_log.end_pass("prediction")
        labels = [int(y) if y >= 0 else None for y in torch.cat(labels_l).view(-1).tolist()]  # -1: unlabelled
        ids = [ds.ids[i] for i in range(n)] if in_order and hasattr(ds, "ids") else [None] * n
        metrics = None
        if n and all(y is not None for y in labels):
            classes = int(logits.shape[1])
            if max(labels) >= classes:
                raise ValueError(f"predict: label {max(labels)} with {classes} classes")
            cm = torch.bincount(torch.tensor(labels) * classes + preds, minlength=classes * classes).view(classes, classes)  # host
            metrics = metrics_from_confusion(cm.numpy())
            self.logger.info("***** Prediction results *****")
            for key in sorted(metrics.keys()):
                if key not in ("confusion", "per_class"):
                    self.logger.info("  %s = %s", key, str(metrics[key]))
            log_per_class(self.logger, metrics)
        else:
            self.logger.info("***** Prediction results *****: not every sample is labelled, no metrics computed")
        self.logger.info("prediction throughput: %.1f samples/s (%d samples)", self.samples_per_sec, n)
        if write_path is not None:
            d = os.path.dirname(write_path)
            if d:
                os.makedirs(d, exist_ok=True)
            write_predictions(write_path, ids, labels, preds, probs, paths_text, paths_image)
            self.logger.info("Wrote %d predictions to %s", n, write_path)
        self.model.train()
        return {"ids": ids, "labels": labels, "logits": logits, "probs": probs, "preds": preds, "paths_text": paths_text,
                "paths_image": paths_image, "metrics": metrics, "samples_per_sec": self.samples_per_sec}

    def _step(self, batch, mode="train"):
        input_ids, input_mask, segment_ids, img_mask, labels, images = batch[:6]  # img_mask is unused (train.py:281-284)
        if len(batch) == 6:
            outputs = self.model(input_ids=input_ids, attention_mask=input_mask, token_type_ids=segment_ids,
                                 labels=labels, images=images)
        else:  # a mixed training batch: (..., labels_b, lam) from the mixer
            outputs = self.model(input_ids=input_ids, attention_mask=input_mask, token_type_ids=segment_ids,
                                 labels=labels, images=images, labels_b=batch[6], mix_lam=batch[7])
        return outputs, labels
