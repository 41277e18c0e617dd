"""Checkpoint dictionary {'epoch','model_state','optimizer_state','best_result','best_epoch'} saved
as '<name>.pth' (reference: lib/helpers/save_helper.py:6-45).  DataParallel / DDP wrappers are
unwrapped on save so checkpoints are interchangeable with the reference's.  With a weight average (monosowa_amd/ema.py,
``trainer.ema_decay``) a sixth key, 'ema_state' = ``ModelEMA.state_dict()``, rides along, and with ``trainer.teacher_memory`` a key 'teacher_memory' = ``LabelMemory.state_dict()``; without
either the dictionary is the reference's."""
import logging
import os

import torch
import torch.nn as nn


def unwrap(model):
    return model.module if isinstance(model, (nn.DataParallel, nn.parallel.DistributedDataParallel)) else model


def model_state_to_cpu(model_state):
    out = type(model_state)()
    for k, v in model_state.items():
        out[k] = v.cpu()
    return out


def get_checkpoint_state(model=None, optimizer=None, epoch=None, best_result=None, best_epoch=None, ema=None, memory=None):
    optim_state = optimizer.state_dict() if optimizer is not None else None
    if model is None:
        model_state = None
    elif unwrap(model) is not model:
        model_state = model_state_to_cpu(unwrap(model).state_dict())
    else:
        model_state = model.state_dict()
    state = {"epoch": epoch, "model_state": model_state, "optimizer_state": optim_state,
             "best_result": best_result, "best_epoch": best_epoch}
    if ema is not None:
        ema_state = ema.state_dict()
        if model is not None and unwrap(model) is not model:
            ema_state["module"] = model_state_to_cpu(ema_state["module"])
        state["ema_state"] = ema_state
    if memory is not None:                   # trainer.teacher_memory: the label memory (LabelMemory.state_dict(), N * M * 128 bytes)
        state["teacher_memory"] = memory.state_dict()
    return state


def save_checkpoint(state, filename):
    torch.save(state, "{}.pth".format(filename))


def load_checkpoint(model, optimizer, filename, map_location, logger=None, ema=None, weights="model", memory=None):
    """``weights="ema"``: ``model`` receives the checkpoint's averaged weights (``ema_state["module"]``) instead of ``model_state``;
    KeyError when the file has none.  ``ema`` (a ``ModelEMA`` over ``model``): restored from ``ema_state``; from a checkpoint
    without one it starts over from the loaded weights (``updates = 0``), with one warning.  ``memory`` (a ``LabelMemory``): restored
    from ``teacher_memory``; from a checkpoint without one, or with one of other frames, it starts empty, with one warning."""
    if weights not in ("model", "ema"):
        raise ValueError("load_checkpoint: weights must be 'model' or 'ema', got %r" % (weights,))
    if not os.path.isfile(filename):
        raise FileNotFoundError(filename)
    if logger is not None:
        logger.info("==> Loading from checkpoint '{}'".format(filename))
    checkpoint = torch.load(filename, map_location, weights_only=False)
    epoch = checkpoint.get("epoch", -1)
    best_result = checkpoint.get("best_result", 0.0)
    best_epoch = checkpoint.get("best_epoch", 0.0)
    if weights == "ema":
        if checkpoint.get("ema_state") is None:
            raise KeyError("checkpoint '%s' has no 'ema_state': it was written without trainer.ema_decay" % filename)
        if model is not None:
            unwrap(model).load_state_dict(checkpoint["ema_state"]["module"])
    elif model is not None and checkpoint["model_state"] is not None:
        unwrap(model).load_state_dict(checkpoint["model_state"])
    if ema is not None:
        if checkpoint.get("ema_state") is not None:
            ema.load_state_dict(checkpoint["ema_state"])
        else:
            ema.reset()
            (logger or logging.getLogger(__name__)).warning(
                "checkpoint '%s' has no 'ema_state': the weight average starts from the loaded weights with updates = 0", filename)
    if memory is not None:
        memory.load_state_dict(checkpoint.get("teacher_memory"), logger)
    if optimizer is not None and checkpoint["optimizer_state"] is not None:
        optimizer.load_state_dict(checkpoint["optimizer_state"])
    if logger is not None:
        logger.info("==> Done")
    return epoch, best_result, best_epoch
