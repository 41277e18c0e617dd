"""Epoch loop (reference: lib/helpers/trainer_helper.py -- ``Trainer.__init__`` :15-63, ``train``
:65-114, ``train_one_epoch`` :116-178, ``prepare_targets`` :180-191).  Same constructor signature and
checkpoint naming.  Differences that do not change results:

* ``torch.distributed`` aware: under ``torchrun`` the model is wrapped in DistributedDataParallel
  (bucketed RCCL all-reduce overlapped with backward); rank 0 alone writes checkpoints and logs.
* the per-iteration ``.item()`` of ~30 loss terms (a host sync every step, :153-157) happens only on
  the logging iterations (every 30th, as printed by the reference).
* with ``optimizer.clip_max_norm`` / ``optimizer.skip_nonfinite`` configured (optimizer_helper.py) the logging iterations
  also print the gradient norm and the number of skipped steps, and an epoch in which EVERY step was skipped raises
  instead of writing a checkpoint; without the keys the printed lines are the reference's.
* ``trainer.global_batch: N`` (optional, absent from the shipped config): N images per optimizer step whatever the number of
  GPUs, by gradient accumulation over K = N / (world size * per-GPU batch) loader batches -- one *cycle*.  A cycle is, by
  definition, one DDP step of K * W ranks: see ``Trainer.train_cycle``.  Absent, 0 or K = 1: the loop below is the plain one.
* ``trainer.ema_decay: X`` (optional, absent from the shipped config; ``trainer.ema_warmup``, default true): an exponential moving
  average of the weights (monosowa_amd/ema.py), updated once per optimizer step right behind it.  The evaluation after an epoch then
  runs on the averaged weights, so ``checkpoint_best`` follows them, and every checkpoint carries an ``ema_state`` beside
  ``model_state``.  Absent, None or 0: nothing is built, allocated, launched or saved.  Under DDP every rank keeps its own copy
  (parameters are bitwise equal across ranks after the all-reduce, so the copies are); rank 0 saves; no collective is added.
* ``trainer.history: true`` (optional, absent from the shipped config): a per-step record kept on the device (monosowa_amd/history.py) --
  every loss term, per module group the gradient norm, the parameter norm and the number of non-finite gradient elements, the guard's
  verdict -- without a synchronisation in the step.  It is read once per epoch, behind the guard check: every rank drains (under DDP
  the loss columns are averaged over the ranks by ONE all-reduce of the ring; the norm columns are equal across ranks), rank 0 appends
  one JSON object per step to ``<output_dir>/history.jsonl`` (truncated when a run starts without ``resume_model``, appended to with
  it; non-finite numbers as the strings "nan", "inf", "-inf") and logs the epoch means of the weighted loss terms, the median and
  maximum of the global gradient norm and one line per step that had non-finite gradients.  Absent, None or false: nothing is built,
  allocated, launched, written or logged; nothing is added to a checkpoint either way.
* ``trainer.label_audit: true`` (optional, absent from the shipped config): a per-label record kept on the device
  (monosowa_amd/label_audit.py) -- for every label of every batch the mean of each matched-pair loss term over its ``group_num`` pairs of
  the final decoder layer, the matched queries' score and the number of pairs -- by one launch per forward, without a synchronisation in
  the step.  It describes the forward, so a step the guard skipped is recorded like any other.  It is read once per epoch, beside the
  history: every rank writes ``<output_dir>/label_audit/epoch_%03d.npz`` (``epoch_%03d.rankR.npz`` under DDP; no collective is added)
  and rank 0 logs the number of labels seen and the median and maximum of their |d - d*|.  ``tools/label_audit.py report`` ranks the
  labels over the epochs.  Absent, None or false: nothing is built, allocated, launched, written or logged; the checkpoint is the same
  either way.
* ``trainer.teacher: {...}`` (optional, absent from the shipped config; keys ``refresh``, ``source``, ``per_step``, ``min_score``,
  ``weights``, ``start_epoch`` -- monosowa_amd/teacher.py): a mean teacher labels the raw frames of ``dataset.unlabelled_split`` one cycle
  ahead, and from ``start_epoch`` on every optimizer step is one cycle of the K labelled loader batches followed by ``per_step``
  pseudo-labelled ones, under ``train_cycle``'s rules for the whole cycle.  At the top of a cycle: collect the batches submitted
  during the previous cycle (the only wait: a slot event recorded before that cycle's kernels), refresh the teacher's weights when
  ``refresh`` optimizer steps have passed (the first cycle of a run refreshes), submit the next cycle's batches, run the cycle.  The
  ``Teacher`` is built by the caller from the whole configuration and handed over as ``teacher=``.  Absent or None: nothing is built,
  allocated, launched or logged; nothing is added to a checkpoint either way.
* ``trainer.teacher_memory: {...}`` (optional sibling of ``trainer.teacher``; keys ``momentum``, ``iou``, ``drop_below``, ``slots`` --
  monosowa_amd/teacher_memory.py): that Teacher keeps a per-frame label memory on the device and encodes the memory's rows; the pseudo
  log line gains the memory's tallies and every checkpoint the key ``teacher_memory``.  Absent or None: nothing of this.
"""
import contextlib
import math
import os

import numpy as np
import torch
import tqdm

from ..image_prep import is_raw_batch, prepare
from ..monodetr import misc
from ..monodetr.criterion import weighted_total
from ..synthetic import attach_host_any, attach_host_mask, attach_host_weight, host_label_weight
from ..synthetic import prepare_targets as _prepare_targets
from .save_helper import get_checkpoint_state, load_checkpoint, save_checkpoint, unwrap


def wrap_ddp(model, device):
    """DDP with few large buckets (xGMI rings are per-link bound) and the never-used parameters frozen."""
    force = os.environ.get("MONOSOWA_FORCE_DDP") == "1"        # rehearse the DDP path on a 1-GPU box
    if not (misc.is_dist_avail_and_initialized() and (misc.get_world_size() > 1 or force)):
        return model
    core = unwrap(model)
    unused = set(core.unused_parameter_names()) if hasattr(core, "unused_parameter_names") else set()
    for n, p in core.named_parameters():
        if n in unused:
            p.requires_grad_(False)
    ids = [device.index] if device.type == "cuda" else None
    return torch.nn.parallel.DistributedDataParallel(core, device_ids=ids, bucket_cap_mb=64,
                                                     gradient_as_bucket_view=True, broadcast_buffers=False)


_EVAL_WAIT_GROUP = []


def wait_for_evaluation(timeout_hours=6.0):
    """All ranks meet here after rank 0's checkpoint / evaluation block: a barrier on a dedicated gloo group (host-side, created
    on first use by every rank at the same point of the epoch loop) whose timeout covers a whole KITTI val inference + AP run."""
    import datetime
    if not _EVAL_WAIT_GROUP:
        _EVAL_WAIT_GROUP.append(torch.distributed.new_group(backend="gloo", timeout=datetime.timedelta(hours=timeout_hours)))
    torch.distributed.monitored_barrier(group=_EVAL_WAIT_GROUP[0], timeout=datetime.timedelta(hours=timeout_hours))


def stage_batch(raw, device):
    """One collated loader batch ``(inputs, calibs, targets, info)`` onto ``device`` (reference: trainer_helper.py:121-127, a
    per-key ``.to(device)``): non-blocking copies (pinned source buffers when the loader pins), images to channels-last for the
    MIOpen NHWC kernels, and the object mask kept on the host next to its device copy so that ``prepare_targets`` needs no
    device -> host synchronisation.  A raw batch (dataset.device_aug: uint8 images on one canvas, records in ``info["prep"]``) is
    copied as it is and becomes the same float32 channels-last images through one launch of monosowa_amd/image_prep.py."""
    inputs, calibs, targets, info = raw
    if is_raw_batch(inputs):
        inputs = prepare(inputs, info["prep"], device)
    else:
        inputs = inputs.to(device, non_blocking=True)
        if inputs.is_cuda:
            inputs = inputs.contiguous(memory_format=torch.channels_last)
    calibs = calibs.to(device, non_blocking=True)
    host_mask = targets["mask_2d"].numpy() if not targets["mask_2d"].is_cuda else None
    host_weight = targets["label_weight"].numpy() if "label_weight" in targets and not targets["label_weight"].is_cuda else None
    host_ignore = bool(targets["ignore_mask"].any()) if "ignore_mask" in targets and not targets["ignore_mask"].is_cuda else None
    targets = {k: v.to(device, non_blocking=True) for k, v in targets.items()}
    if host_ignore is not None:
        attach_host_any(targets["ignore_mask"], host_ignore)          # a batch without an ignore box is a batch without the keys
    if host_mask is not None:
        attach_host_mask(targets["mask_2d"], host_mask)      # prepare_targets then needs no device sync
    if host_weight is not None:
        attach_host_weight(targets["label_weight"], host_weight)      # nor does the weighted normaliser
    return inputs, calibs, targets, info


class Trainer(object):
    def __init__(self, cfg, model, optimizer, train_loader, test_loader, lr_scheduler, warmup_lr_scheduler,
                 logger, loss, model_name, teacher=None):
        self.cfg = cfg
        self.optimizer = optimizer
        self.train_loader = train_loader
        self.test_loader = test_loader
        self.lr_scheduler = lr_scheduler
        self.warmup_lr_scheduler = warmup_lr_scheduler
        self.logger = logger
        self.epoch = 0
        self.best_result = 0
        self.best_epoch = 0
        if torch.cuda.is_available():
            self.device = torch.device("cuda", torch.cuda.current_device())
        else:
            self.device = torch.device("cpu")
        if self.device.type == "cuda":
            from .model_helper import to_mi355x_layout
            to_mi355x_layout(unwrap(model))
        self.model = wrap_ddp(model, self.device)
        self.detr_loss = loss
        self.model_name = model_name
        self.output_dir = os.path.join("./" + cfg["save_path"], model_name)
        self.tester = None
        self.log_interval = 30
        self._guard_skipped = 0          # optimizer.guard_report()["skipped_total"] at the end of the previous epoch
        self.accum_steps = self._accum_steps(cfg.get("global_batch"), train_loader)      # K: loader batches per optimizer step
        self._accumulator = None
        ema_decay = self._ema_decay(cfg.get("ema_decay"))
        self.ema = None                  # ModelEMA with trainer.ema_decay, built below once the weights are the ones training starts from
        history = self._history_flag(cfg.get("history"))
        self.history = None              # StepHistory with trainer.history, built below once the model is where it trains
        self._history_step = 0           # optimizer steps committed in the current epoch
        self._history_fresh = not cfg.get("resume_model", None)      # the first write of this run truncates history.jsonl
        label_audit = self._label_audit_flag(cfg.get("label_audit"))
        self.label_audit = None          # LabelAudit with trainer.label_audit, built below on the device the model trains on
        self.teacher_cfg = self._teacher_config(cfg.get("teacher"), ema_decay is not None, label_audit, teacher)
        self.teacher = teacher           # monosowa_amd.Teacher with trainer.teacher, built by the caller from the whole configuration
        self._teacher_cycles = 0         # cycles of this run with the teacher on: it refreshes when this is a multiple of `refresh`
        self._pseudo_counts = (0, 0)     # (targets, ignore boxes) of the pseudo batches of the cycle collected last
        self._memory_counts = None       # trainer.teacher_memory: that cycle's (matched, created, missed, dropped, evicted) sums
        if cfg.get("teacher_memory") is not None and self.teacher_cfg is None:
            from ..teacher_memory import memory_config
            memory_config(cfg["teacher_memory"], None)     # malformed, or the key without trainer.teacher: ValueError

        if cfg.get("pretrain_model"):
            assert os.path.exists(cfg["pretrain_model"])
            load_checkpoint(model=self.model, optimizer=None, filename=cfg["pretrain_model"],
                            map_location=self.device, logger=self.logger)
        resume = os.path.join(self.output_dir, "checkpoint.pth") if cfg.get("resume_model", None) else None
        if resume is not None:
            assert os.path.exists(resume)
            self.model.to(self.device)
        if ema_decay is not None:
            # after the layout change and the moves above: every averaged tensor has its parameter's strides and device
            from ..ema import ModelEMA
            self.ema = ModelEMA(self.model, ema_decay, warmup=bool(cfg.get("ema_warmup", True)))
        if history:
            from ..history import StepHistory
            steps = -(-len(train_loader) // self.accum_steps)          # optimizer steps of an epoch: never a drain inside one
            self.history = StepHistory(self.model, self.detr_loss.weight_dict, max(steps, 1))
        if label_audit:
            from ..label_audit import LabelAudit
            self.label_audit = LabelAudit(self._label_audit_rows(train_loader), self.device)
            self.detr_loss.audit = self.label_audit
        if self.teacher is not None:
            self.teacher.bind_source(self.ema)
        if resume is not None:
            self.epoch, self.best_result, self.best_epoch = load_checkpoint(
                model=self.model, optimizer=self.optimizer, filename=resume,
                map_location=self.device, logger=self.logger, ema=self.ema, **self._memory_argument())
            self.lr_scheduler.last_epoch = self.epoch - 1
            self.logger.info("Loading Checkpoint... Best Result:{}, Best Epoch:{}".format(self.best_result, self.best_epoch))

    def train(self):
        try:
            return self._train()
        finally:
            if self.teacher is not None:                   # in-flight batches, the engine's graphs, the unlabelled loader's workers
                self.teacher.close()

    def _train(self):
        start_epoch = self.epoch
        best_result, best_epoch = self.best_result, self.best_epoch
        main = misc.is_main_process()
        if self.history is not None and main:
            self._history_file()                           # a run without resume_model starts from an empty file
        bar = tqdm.tqdm(range(start_epoch, self.cfg["max_epoch"]), dynamic_ncols=True, leave=True, desc="epochs", disable=not main)
        for epoch in range(start_epoch, self.cfg["max_epoch"]):
            np.random.seed(np.random.get_state()[1][0] + epoch)
            sampler = getattr(self.train_loader, "sampler", None)
            if hasattr(sampler, "set_epoch"):
                sampler.set_epoch(epoch)
            self.train_one_epoch(epoch)
            self.epoch += 1
            if self.warmup_lr_scheduler is not None and epoch < 5:
                self.warmup_lr_scheduler.step()
            else:
                self.lr_scheduler.step()
            if (self.epoch % self.cfg["save_frequency"]) == 0 and main:
                os.makedirs(self.output_dir, exist_ok=True)
                name = "checkpoint_epoch_%d" % self.epoch if self.cfg["save_all"] else "checkpoint"
                save_checkpoint(self._checkpoint_state(best_result, best_epoch), os.path.join(self.output_dir, name))
                if self.tester is not None:
                    self.logger.info("Test Epoch {}".format(self.epoch) + (" (EMA weights)" if self.ema is not None else ""))
                    cur = self._evaluate()
                    if cur > best_result:
                        best_result, best_epoch = cur, self.epoch
                        save_checkpoint(self._checkpoint_state(best_result, best_epoch), os.path.join(self.output_dir, "checkpoint_best"))
                    self.logger.info("Best Result:{}, epoch:{}".format(best_result, best_epoch))
            if (self.epoch % self.cfg["save_frequency"]) == 0 and misc.is_dist_avail_and_initialized():
                # rank 0 saved / evaluated alone: the other ranks wait here instead of inside the next epoch's first
                # gradient all-reduce.  The wait runs on its own gloo group with a timeout sized for a full validation pass
                # (the default group's collective timeout -- 10 minutes under RCCL -- would abort a long evaluation just the
                # same, only inside this barrier)
                wait_for_evaluation()
            bar.update()
        self.logger.info("Best Result:{}, epoch:{}".format(best_result, best_epoch))
        return None

    def _memory_argument(self):
        """``{"memory": the teacher's LabelMemory}`` with ``trainer.teacher_memory``, else nothing: the calls are today's."""
        memory = getattr(self.teacher, "memory", None)
        return {} if memory is None else {"memory": memory}

    def _checkpoint_state(self, best_result, best_epoch):
        if self.ema is None:
            return get_checkpoint_state(self.model, self.optimizer, self.epoch, best_result, best_epoch, **self._memory_argument())
        return get_checkpoint_state(self.model, self.optimizer, self.epoch, best_result, best_epoch, ema=self.ema,
                                    **self._memory_argument())

    def _evaluate(self):
        """The tester's pass after an epoch; with the weight average on, over the averaged weights: the tester's model is swapped for
        the pass and put back afterwards, whatever happens."""
        if self.ema is None:
            self.tester.inference()
            return self.tester.evaluate()
        live = self.tester.model
        self.tester.model = self.ema.sync_untracked()
        try:
            self.tester.inference()
            return self.tester.evaluate()
        finally:
            self.tester.model = live

    @staticmethod
    def _ema_decay(value):
        """``trainer.ema_decay``: None for absent, None or 0 (off), else the decay, a number inside (0, 1)."""
        if value is None or (not isinstance(value, bool) and isinstance(value, (int, float)) and value == 0):
            return None
        if isinstance(value, bool) or not isinstance(value, (int, float)) or not 0.0 < float(value) < 1.0:
            raise ValueError("trainer.ema_decay = %r is not a number inside (0, 1) (absent, None or 0: off)" % (value,))
        return float(value)

    @staticmethod
    def _history_flag(value):
        """``trainer.history``: False for absent, None or false, True for true; anything else is refused."""
        if value is None:
            return False
        if not isinstance(value, bool):
            raise ValueError("trainer.history = %r is not a bool (absent, None or false: off)" % (value,))
        return value

    @staticmethod
    def _label_audit_flag(value):
        """``trainer.label_audit``: False for absent, None or false, True for true; anything else is refused."""
        if value is None:
            return False
        if not isinstance(value, bool):
            raise ValueError("trainer.label_audit = %r is not a bool (absent, None or false: off)" % (value,))
        return value

    @staticmethod
    def _teacher_config(value, ema_on, label_audit, teacher):
        """``trainer.teacher``: None for absent or None (off), else the checked ``TeacherConfig``; the key and the ``teacher=``
        argument come together or not at all."""
        if value is None:
            if teacher is not None:
                raise ValueError("Trainer(teacher=...) without trainer.teacher in the configuration")
            return None
        from ..teacher import teacher_config
        checked = teacher_config(value, ema_on, getattr(teacher, "threshold", None))
        if label_audit:
            raise ValueError("trainer.label_audit names every label by its label line: pseudo rows have none, so it cannot be "
                             "combined with trainer.teacher")
        if teacher is None:
            raise ValueError("trainer.teacher is set: build monosowa_amd.Teacher from the whole configuration and pass it as teacher=")
        return checked

    @staticmethod
    def _label_audit_rows(train_loader):
        """Rows of the audit's ring: the labels an epoch can hold, so that the ring is never drained inside one -- ``len(dataset) x
        max_objs`` when the loader exposes both, else the loader's ``len x batch_size x 50``."""
        dataset = getattr(train_loader, "dataset", None)
        max_objs = getattr(dataset, "max_objs", None)
        if dataset is not None and isinstance(max_objs, int) and max_objs > 0 and hasattr(dataset, "__len__"):
            return max(len(dataset) * max_objs, 1)
        return max(len(train_loader) * int(getattr(train_loader, "batch_size", None) or 1) * 50, 1)

    def _drain_label_audit(self, epoch):
        """End of an epoch with ``trainer.label_audit``: the ring to the host (the one synchronisation of the record), every rank
        writes its own file, rank 0 logs the summary.  No collective."""
        from ..label_audit import COLUMNS, save
        record = self.label_audit.drain()
        ranked = misc.is_dist_avail_and_initialized() and misc.get_world_size() > 1
        name = "epoch_%03d.rank%d.npz" % (epoch, misc.get_rank()) if ranked else "epoch_%03d.npz" % epoch
        save(os.path.join(self.output_dir, "label_audit", name), record)
        if not misc.is_main_process():
            return
        err = record["values"][:, COLUMNS.index("depth_abs")]
        if len(err):
            with np.errstate(invalid="ignore"):
                self.logger.info("Epoch {}: label audit: {} labels seen, |d - d*| median: {:.4g}, max: {:.4g}".format(
                    epoch, len(err), float(np.median(err)), float(np.max(err))))
        else:
            self.logger.info("Epoch {}: label audit: 0 labels seen".format(epoch))

    def _history_commit(self, micro_batches):
        self.history.commit(self.optimizer, epoch=self.epoch, step=self._history_step, lr=self.optimizer.param_groups[0]["lr"],
                            micro_batches=micro_batches)
        self._history_step += 1

    def _history_file(self):
        """Path of ``history.jsonl``; the first call of a run without ``resume_model`` leaves the file empty."""
        path = os.path.join(self.output_dir, "history.jsonl")
        if self._history_fresh:
            os.makedirs(self.output_dir, exist_ok=True)
            open(path, "w").close()
            self._history_fresh = False
        return path

    def _drain_history(self, epoch):
        """End of an epoch with ``trainer.history``: the ring to the host (the one synchronisation of the record; every rank takes
        part in the all-reduce of the loss columns), rank 0 appends to ``history.jsonl`` and logs the epoch's summary."""
        from ..history import to_json
        rows = self.history.drain()
        self._history_step = 0
        if not misc.is_main_process():
            return
        path = self._history_file()
        os.makedirs(self.output_dir, exist_ok=True)
        with open(path, "a") as f:
            for row in rows:
                f.write(to_json(row) + "\n")
        weight_dict = self.detr_loss.weight_dict
        finite = [r for r in rows if math.isfinite(r["loss_detr"])]
        if finite:
            means = {k: float(np.mean([r["losses"][k] for r in finite])) * float(weight_dict[k]) for k in finite[0]["losses"]}
            self.logger.info("Epoch {}: mean over {} of {} steps: loss_detr: {:.4f}, ".format(
                epoch, len(finite), len(rows), float(np.mean([r["loss_detr"] for r in finite])))
                + ", ".join("%s: %.4f" % kv for kv in means.items()))
        else:
            self.logger.info("Epoch {}: mean over 0 of {} steps: no step with a finite loss_detr".format(epoch, len(rows)))
        if rows:
            with np.errstate(invalid="ignore", over="ignore"):
                norms = [float(np.sqrt(np.sum(np.square(list(r["grad_norm"].values()))))) for r in rows]
            self.logger.info("Epoch {}: grad_norm median: {:.4g}, max: {:.4g}".format(epoch, float(np.median(norms)), float(np.max(norms))))
        for r in rows:
            bad = {g: n for g, n in r["grad_nonfinite"].items() if n > 0}
            if bad:
                skipped = "skipped" if r.get("guard", {}).get("skip") else "not skipped"
                self.logger.info("Epoch {} step {}: non-finite gradients ({}): {}".format(
                    epoch, r["step"], skipped, ", ".join("%s: %d" % kv for kv in bad.items())))

    def train_step(self, inputs, calibs, targets, info=None):
        """One optimizer step on a device-resident batch; returns (total loss tensor, loss dict)."""
        img_sizes = targets["img_size"]
        target_list = self.prepare_targets(targets, inputs.shape[0])
        if self.label_audit is not None:
            self._audit_begin(targets, info, inputs.shape[0])
        self.optimizer.zero_grad(set_to_none=True)
        outputs = self.model(inputs, calibs, target_list, img_sizes, dn_args=None)
        loss_dict = self.detr_loss(outputs, target_list, None, info)
        weight_dict = self.detr_loss.weight_dict
        total = weighted_total(loss_dict, weight_dict)
        total.backward()
        if self.history is not None:
            self.history.add_losses(loss_dict, total)
        self.optimizer.step()
        if self.history is not None:
            self._history_commit(1)
        if self.ema is not None:
            self.ema.update(self.optimizer)
        return total, loss_dict

    def _audit_begin(self, targets, info, batch_size):
        """Reserves the audit's rows for the forward that follows and names them: ``info["img_id"]`` and the host object mask."""
        if info is None or "img_id" not in info:
            raise ValueError("trainer.label_audit names every label by its image: the batch's info needs \"img_id\"")
        self.label_audit.begin_batch(np.asarray(info["img_id"]).reshape(-1)[:batch_size], targets["mask_2d"], epoch=self.epoch)

    @staticmethod
    def _accum_steps(global_batch, train_loader):
        """K of ``trainer.global_batch: N``: N / (W * b), W the world size and b the loader's per-GPU batch size; 1 without the key."""
        if not global_batch:             # absent, None or 0: off
            return 1
        world, per_gpu = misc.get_world_size(), getattr(train_loader, "batch_size", None)
        ok = isinstance(global_batch, int) and not isinstance(global_batch, bool) and isinstance(per_gpu, int) and per_gpu > 0 \
            and global_batch > 0 and global_batch % (world * per_gpu) == 0
        if not ok:
            raise ValueError("trainer.global_batch = %r is not a positive multiple of world size x per-GPU batch size = %r x %r"
                             % (global_batch, world, per_gpu))
        return global_batch // (world * per_gpu)

    @staticmethod
    def _host_box_count(raw):
        """Boxes of one collated loader batch, from the object mask on the host (no device synchronisation); with ``label_weight`` in
        the targets the sum of the boxes' weights (a float)."""
        mask = raw[2]["mask_2d"]
        host = getattr(mask, "_host_mask", None)
        if host is None:
            if mask.is_cuda:
                raise ValueError("gradient accumulation counts the boxes of a cycle on the host: a device-resident batch needs "
                                 "synthetic.attach_host_mask on its mask_2d")
            host = mask.numpy()
        if "label_weight" in raw[2]:               # dataset.label_weights: the boxes count with their weights
            from ..monodetr.criterion import label_weight_sum
            return label_weight_sum(host_label_weight(raw[2]), host)
        return int(np.count_nonzero(host))

    def _cycle_num_boxes(self, n_boxes, micro_steps):
        """The criterion's normaliser for every micro-batch of a cycle with ``n_boxes`` boxes on this rank:
        max(job-wide boxes * group_num / (K * W), 1) -- ``SetCriterion._num_boxes`` with K * W in place of the world size."""
        group_num = self.detr_loss.group_num if self.detr_loss.training else 1
        n = float(n_boxes * group_num)
        ranks = micro_steps * misc.get_world_size()
        if misc.is_dist_avail_and_initialized():           # one all-reduce per cycle, on the device: no sync
            t = torch.as_tensor(np.asarray([n])).to(torch.float).to(self.device, non_blocking=True)
            torch.distributed.all_reduce(t)
            return torch.clamp(t / ranks, min=1)[0]
        return max(n / ranks, 1.0)

    def _teacher_turn(self):
        """The top of a cycle with the teacher on: the staged pseudo batches of THIS cycle (submitted during the previous one; none
        in the first), then the refresh when it is due, then the next cycle's submissions."""
        t, c = self.teacher, self.teacher_cfg
        staged, targets, ignored = [], 0, 0
        remembered = None if getattr(t, "memory", None) is None else [0] * 5
        while t.in_flight():
            staged.append(t.collect())
            targets, ignored = targets + t.last_counts[0], ignored + t.last_counts[1]
            if remembered is not None:
                remembered = [a + b for a, b in zip(remembered, t.last_memory)]
        self._pseudo_counts = (targets, ignored)           # of the whole cycle (per_step batches), from the pinned copies
        self._memory_counts = None if remembered is None else tuple(remembered)
        if self._teacher_cycles % c.refresh == 0:
            t.refresh()
        self._teacher_cycles += 1
        for _ in range(c.per_step):
            t.submit(t.next_raw())
        return staged

    def train_cycle(self, raws, staged=()):
        """One optimizer step over the K = len(raws) collated loader batches of a cycle; returns the last micro-batch's (total loss
        tensor, loss dict).  Defined as one DDP step of K * W ranks (W the world size), rank by rank: every micro-batch has its own
        forward (its own matching and size compensation) and is normalised by the box count of the whole cycle over all ranks,
        max(n * group_num / (K * W), 1); its weighted loss enters with 1 / K, which is DDP's gradient mean.  The gradients add up in
        micro-batch order, one float32 add per element and micro-step; the optimizer (and its guard) sees the sum once.  Under DDP
        only the last backward all-reduces.  The staged copy of a batch lives for its own micro-step only.  With ``trainer.history`` the
        row of the cycle holds sum_k term_k / K for every raw loss term (``add_losses`` with scale 1 / K) and sum_k total_k for
        ``loss_detr``: ``total`` carries its 1 / K already and is added as it is.  ``staged`` (``trainer.teacher``): pseudo-labelled
        micro-batches, already on the device, that follow the labelled ones as further micro-batches of the same cycle: K counts
        them too."""
        K = len(raws) + len(staged)
        if K == 1 and not staged:                          # the tail of an epoch: exactly a plain step
            return self.train_step(*stage_batch(raws[0], self.device))
        num_boxes = self._cycle_num_boxes(sum(self._host_box_count(raw) for raw in list(raws) + list(staged)), K)
        ddp = isinstance(self.model, torch.nn.parallel.DistributedDataParallel)
        if self._accumulator is None:
            from ..pointwise import GradAccumulator
            # DDP's gradients are views of its buckets: there autograd adds in place, inside no_sync()
            self._accumulator = GradAccumulator([p for g in self.optimizer.param_groups for p in g["params"]], fused=not ddp)
        acc = self._accumulator
        acc.begin()
        weight_dict = self.detr_loss.weight_dict
        self.optimizer.zero_grad(set_to_none=True)
        for k in range(K):
            inputs, calibs, targets, info = stage_batch(raws[k], self.device) if k < len(raws) else staged[k - len(raws)]
            target_list = self.prepare_targets(targets, inputs.shape[0])
            if self.label_audit is not None:
                self._audit_begin(targets, info, inputs.shape[0])
            with (self.model.no_sync() if ddp and k < K - 1 else contextlib.nullcontext()):
                outputs = self.model(inputs, calibs, target_list, targets["img_size"], dn_args=None)
                loss_dict = self.detr_loss(outputs, target_list, None, info, num_boxes=num_boxes)
                total = weighted_total(loss_dict, weight_dict) / K
                total.backward()
            if self.history is not None:
                self.history.add_losses(loss_dict, total, scale=1.0 / K)
            acc.collect(k)
        acc.install()
        self.optimizer.step()
        if self.history is not None:
            self._history_commit(K)
        if self.ema is not None:
            self.ema.update(self.optimizer)
        return total, loss_dict

    def train_one_epoch(self, epoch):
        torch.set_grad_enabled(True)
        self.model.train()
        self.detr_loss.train()
        main = misc.is_main_process()
        if main:
            print(">>>>>>> Epoch:", str(epoch) + ":")
        bar = tqdm.tqdm(total=len(self.train_loader), leave=(self.epoch + 1 == self.cfg["max_epoch"]), desc="iters", disable=not main)
        steps = 0
        teaching = self.teacher is not None and epoch >= self.teacher_cfg.start_epoch
        if self.accum_steps > 1 or teaching:
            raws = []

            def cycle():
                nonlocal steps, raws
                total, loss_dict = self.train_cycle(raws, self._teacher_turn()) if teaching else self.train_cycle(raws)
                if steps % self.log_interval == 0:             # every log_interval-th optimizer step
                    self._log(steps, loss_dict)
                    if teaching and misc.is_main_process():
                        line = "pseudo: targets %d, ignored %d" % self._pseudo_counts
                        if self._memory_counts is not None:
                            line += ", memory: matched %d, created %d, missed %d, dropped %d, evicted %d" % self._memory_counts
                        print(line + "\n")
                steps += 1
                bar.update(len(raws))
                raws = []
            for raw in self.train_loader:
                raws.append(raw)                           # collated batches wait on the host; one at a time is staged
                if len(raws) == self.accum_steps:
                    cycle()
            if raws:                                       # the epoch's tail: len(loader) mod K micro-batches
                cycle()
        else:
            for batch_idx, raw in enumerate(self.train_loader):
                inputs, calibs, targets, info = stage_batch(raw, self.device)
                total, loss_dict = self.train_step(inputs, calibs, targets, info)
                steps += 1
                if batch_idx % self.log_interval == 0:
                    self._log(batch_idx, loss_dict)
                bar.update()
        bar.close()
        # the device assignment solver reports an invalid cost matrix through a status word (no exception from a kernel, no wait in
        # the step): look at it for certain before the epoch's checkpoint is written
        matcher = getattr(self.detr_loss, "matcher", None)
        if matcher is not None and hasattr(matcher, "check_device_status"):
            matcher.check_device_status(block=True)
        try:
            self._check_guard(epoch, steps)
        finally:
            if self.history is not None:                   # an epoch the guard refuses is the one whose record is wanted
                self._drain_history(epoch)
            if self.label_audit is not None:
                self._drain_label_audit(epoch)

    def _guard_report(self):
        """The optimizer's guard record when the guarded step is configured (a host synchronisation), else None."""
        if not getattr(self.optimizer, "guard_enabled", False):
            return None
        return self.optimizer.guard_report()

    def _check_guard(self, epoch, steps):
        """End of an epoch under the guarded step: how many of its steps were skipped for non-finite gradients; all of them means
        the model is not training, and the epoch's checkpoint must not look healthy."""
        report = self._guard_report()
        if report is None:
            return
        skipped = report["skipped_total"] - self._guard_skipped
        self._guard_skipped = report["skipped_total"]
        self.logger.info("Epoch {}: {} of {} steps skipped (non-finite gradients)".format(epoch, skipped, steps))
        if steps > 0 and skipped >= steps:
            raise RuntimeError("every step of epoch %d (%d) was skipped for non-finite gradients: the model is not training" % (epoch, steps))

    def _log(self, batch_idx, loss_dict):
        weight_dict = self.detr_loss.weight_dict
        reduced = misc.reduce_dict({k: v for k, v in loss_dict.items() if k in weight_dict})
        if not misc.is_main_process():
            return
        logged = {k: (reduced[k] * weight_dict[k]).item() for k in reduced}
        print("----", batch_idx, "----")
        print("%s: %.2f, " % ("loss_detr", sum(logged.values())))
        seen = set()
        for key, val in logged.items():
            if key[-1].isdigit() and key[-1] not in seen:
                print("")
                seen.add(key[-1])
            print("%s: %.2f, " % (key, val), end="")
        print("\n")
        report = self._guard_report()
        if report is not None:
            print("grad_norm: %.4g, skipped: %d\n" % (report["grad_norm"], report["skipped_total"]))
        ignore = self.detr_loss.ignore_report() if hasattr(self.detr_loss, "ignore_report") else None
        # model.ignore_depth_map: depth-map pixels left out of loss_depth_map in this step (None with the key off)
        px = self.detr_loss.ignore_depth_report() if hasattr(self.detr_loss, "ignore_depth_report") else None
        px_text = "" if px is None else "ignored px: %d of %d" % px
        if ignore is not None:                             # dataset.ignore_regions: queries left out of loss_ce in this step, all layers
            print("ignored: %d of %d%s\n" % (sum(ignore[0]), len(ignore[0]) * ignore[1], ", " + px_text if px_text else ""))
        elif px_text:
            print(px_text + "\n")

    @staticmethod
    def prepare_targets(targets, batch_size):
        return _prepare_targets(targets, batch_size)
