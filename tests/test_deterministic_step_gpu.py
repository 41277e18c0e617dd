"""Whole train steps of the shipped model under torch.use_deterministic_algorithms(True), in child processes
(tools/deterministic_step.py): 2 AdamW steps on the synthetic KITTI-size batch give bit-identical losses, gradients and
updated parameters -- twice in one process, across two fresh processes, and under DistributedDataParallel at world size 1
against the unwrapped model (the exact check tests/test_ddp_gpu.py cannot make in the default mode)."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "deterministic_step.py")


def _child(mode, env_extra=None, timeout=600):
    env = dict(os.environ, **(env_extra or {}))
    r = subprocess.run([sys.executable, TOOL, mode], env=env, capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    if r.returncode != 0:
        pytest.fail("%s child failed (rc %d)\n--- stdout ---\n%s\n--- stderr ---\n%s"
                    % (mode, r.returncode, r.stdout[-2000:], r.stderr[-6000:]), pytrace=False)
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_two_runs_in_one_process_are_bit_identical():
    res = _child("repeat")
    assert res["n_tensors"] > 600 and res["differ"] == [], res["differ"][:20]


def test_two_processes_give_the_same_digest():
    a = _child("digest")
    b = _child("digest")
    assert a["n_tensors"] == b["n_tensors"] > 600
    assert a["sha256"] == b["sha256"], (a, b)


def test_ddp_world_size_1_is_bit_identical_to_the_unwrapped_model():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    res = _child("ddp", {"MONOSOWA_FORCE_DDP": "1", "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port), "RANK": "0",
                         "WORLD_SIZE": "1", "LOCAL_RANK": "0", "HSA_ENABLE_IPC_MODE_LEGACY": "0"})
    assert res["n_tensors"] > 600 and res["differ"] == [], res["differ"][:20]
