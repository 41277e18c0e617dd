"""Logger and seeding (reference: lib/helpers/utils_helper.py:6-26)."""
import logging
import os
import random

import numpy as np
import torch


def create_logger(log_file, rank=0):
    log_format = "%(asctime)s  %(levelname)5s  %(message)s"
    logging.basicConfig(level=logging.INFO if rank == 0 else "ERROR", format=log_format, filename=log_file)
    console = logging.StreamHandler()
    console.setLevel(logging.INFO if rank == 0 else "ERROR")
    console.setFormatter(logging.Formatter(log_format))
    logging.getLogger(__name__).addHandler(console)
    return logging.getLogger(__name__)


def set_deterministic(trainer_cfg):
    """``trainer.deterministic: True`` (optional, default False): bitwise-reproducible training -- the same weights, seed, batch,
    build and device type give the same losses, gradients and parameters.  Turns on ``torch.use_deterministic_algorithms``,
    which the native kernels read at every call (README "Deterministic training"); an op without a deterministic
    implementation then raises.  CUBLAS_WORKSPACE_CONFIG is set (if unset) before the first BLAS call: CUDA builds of torch
    demand it in this mode; the ROCm build measured (torch 2.10, ROCm 7) does not (tools/deterministic_step.py reports it)."""
    if not (trainer_cfg or {}).get("deterministic", False):
        return False
    os.environ.setdefault("CUBLAS_WORKSPACE_CONFIG", ":4096:8")
    torch.use_deterministic_algorithms(True)
    return True


def set_random_seed(seed):
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed ** 2)
    torch.cuda.manual_seed(seed ** 3)
    torch.backends.cudnn.deterministic = True      # MIOpen honours the same switch on ROCm
    torch.backends.cudnn.benchmark = False
