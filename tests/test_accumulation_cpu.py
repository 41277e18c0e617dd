"""``trainer.global_batch``: one optimizer step over K loader batches, defined as one DDP step of K * W ranks.  On the CPU, with
the tiny model of tests/test_distributed_gloo.py (``_build()``: MSDA through the oracle, depth map 12 x 4, dropout 0, 192 x 64,
batch 2, two threads): the accumulated gradient of K = 2 against a real two-rank DDP step on the same two batches, the criterion's
``num_boxes=`` override, W = 2 with K = 2 over gloo, and the shape of the epoch loop.

The depth predictor keeps a hard-coded dropout of 0.1, so every forward is seeded by a pre-hook: 100 + micro-step index on the
accumulating side, 100 + rank on the DDP side (what test_distributed_gloo.py does by hand)."""
import logging
import os
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from test_distributed_gloo import _build, _free_port

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES = (192, 64)
BOXES = {7: 9, 8: 12}                 # boxes of make_batch(2, "cpu", seed=s, resolution=RES)
LOSS_KEYS = ("loss_center", "loss_bbox", "loss_giou", "loss_depth", "loss_dim", "loss_angle", "loss_ce")


class _Loader:
    """What the Trainer needs of a DataLoader: ``batch_size``, ``len`` and collated batches."""

    def __init__(self, seeds, batch_size=2):
        from monosowa_amd.synthetic import make_batch
        self.batch_size = batch_size
        self.batches = [make_batch(batch_size, "cpu", seed=s, resolution=RES) for s in seeds]

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        return iter(self.batches)


def _count(raw):
    return int(raw[2]["mask_2d"].sum())


def _seed_hook(model):
    """Forward pre-hook seeding torch's generator with 100 + state["k"], then advancing k."""
    state = {"k": 0}

    def hook(module, args):
        torch.manual_seed(100 + state["k"])
        state["k"] += 1
    model.register_forward_pre_hook(hook)
    return state


def _trainer(model, crit, opt, loader, **cfg):
    """A Trainer on the CPU whatever the machine has (the constructor picks the GPU when there is one)."""
    from monosowa_amd.helpers.trainer_helper import Trainer
    available = torch.cuda.is_available
    torch.cuda.is_available = lambda: False
    try:
        trainer = Trainer(dict({"save_path": "outputs", "max_epoch": 1}, **cfg), model, opt, loader, None, None, None,
                          logging.getLogger("test_accumulation"), crit, "tiny")
    finally:
        torch.cuda.is_available = available
    assert trainer.device.type == "cpu"
    return trainer


def _named_grads(model):
    return {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}


def _flat(named, names):
    return torch.cat([named[n].reshape(-1) for n in names])


@pytest.fixture(scope="module", autouse=True)
def _process_state():
    """``_build()`` replaces the MSDA autograd function by the oracle and the tests run on two threads: both are undone."""
    import monosowa_amd.ms_deform_attn_func as F
    fn, threads = F.MSDeformAttnFunction, torch.get_num_threads()
    torch.set_num_threads(2)
    yield
    F.MSDeformAttnFunction = fn
    torch.set_num_threads(threads)


# --------------------------------------------------------------------------------------------------- 1. K = 2 equals two ranks
def _ddp_step_worker(rank, world, port, path):
    """One DDP step, rank r on the batch of seed 7 + r: exactly the set-up of test_distributed_gloo.py."""
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from monosowa_amd.helpers.trainer_helper import wrap_ddp
    from monosowa_amd.monodetr.criterion import weighted_total
    from monosowa_amd.synthetic import make_batch, prepare_targets
    model, crit, opt = _build()
    ddp = wrap_ddp(model, torch.device("cpu"))
    inputs, calibs, targets, _ = make_batch(2, "cpu", seed=7 + rank, resolution=RES)
    tl = prepare_targets(targets, 2)
    torch.manual_seed(100 + rank)
    weighted_total(crit(ddp(inputs, calibs, tl, targets["img_size"]), tl), crit.weight_dict).backward()
    if rank == 0:
        torch.save(_named_grads(model), path)
    dist.barrier()
    dist.destroy_process_group()


def _spawn(worker, path, world=2, timeout=240):
    """Runs ``worker(rank, world, port, path)`` on every rank; rank 0 leaves its result in the file ``path``."""
    port = _free_port()
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=worker, args=(r, world, port, str(path))) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout)
        assert p.exitcode == 0
    return torch.load(str(path))


def test_cycle_of_two_equals_a_two_rank_ddp_step(tmp_path):
    model, crit, opt = _build()
    loader = _Loader([7, 8])
    assert [_count(b) for b in loader.batches] == [BOXES[7], BOXES[8]]       # unequal: a per-micro-batch normaliser cannot pass
    state = _seed_hook(model)
    trainer = _trainer(model, crit, opt, loader, global_batch=4)
    assert trainer.accum_steps == 2
    trainer.model.train(), crit.train()
    state["k"] = 0
    trainer.train_cycle(list(loader))
    acc = _named_grads(model)
    ddp = _spawn(_ddp_step_worker, tmp_path / "ddp.pt")
    assert set(acc) == set(ddp)
    names = sorted(ddp)
    a, d = _flat(acc, names), _flat(ddp, names)
    err, scale = float((a - d).abs().max()), float(d.abs().max())
    print("max|acc - ddp| = %.3e, max|ddp| = %.3e, ratio %.3e" % (err, scale, err / scale))
    assert err <= 1e-4 * scale


# --------------------------------------------------------------------------------------------------- 2. num_boxes= override
@pytest.mark.parametrize("fast", [True, False], ids=["forward_fast", "forward_layerwise"])
def test_num_boxes_override_replaces_the_count_and_the_collective(fast, tmp_path, monkeypatch):
    from monosowa_amd.synthetic import make_batch, prepare_targets
    model, crit, _ = _build()
    crit.fast = fast
    inputs, calibs, targets, _ = make_batch(2, "cpu", seed=7, resolution=RES)
    tl = prepare_targets(targets, 2)
    assert sum(len(t["labels"]) for t in tl) == BOXES[7]
    own = float(BOXES[7] * crit.group_num)
    torch.manual_seed(100)
    with torch.no_grad():
        out = model(inputs, calibs, tl, targets["img_size"])
        base = crit(out, tl)
        for x in (7.5, torch.tensor(7.5)):
            over = crit(out, tl, num_boxes=x)
            for k in LOSS_KEYS + tuple(k + "_0" for k in LOSS_KEYS):
                assert torch.allclose(over[k] * 7.5, base[k] * own, rtol=1e-5), (k, over[k], base[k])
            assert torch.equal(over["loss_depth_map"], base["loss_depth_map"])
        # with a process group up the criterion's own count is all-reduced; the override issues no collective
        dist.init_process_group("gloo", init_method="file://%s" % (tmp_path / "store"), rank=0, world_size=1)
        try:
            def refuse(*args, **kwargs):
                raise AssertionError("all_reduce called")
            monkeypatch.setattr(torch.distributed, "all_reduce", refuse)
            with pytest.raises(AssertionError, match="all_reduce called"):
                crit(out, tl)
            over = crit(out, tl, num_boxes=7.5)
            assert torch.allclose(over["loss_center"] * 7.5, base["loss_center"] * own, rtol=1e-5)
        finally:
            monkeypatch.undo()
            dist.destroy_process_group()


# --------------------------------------------------------------------------------------------------- 3. W = 2, K = 2
W2_SEEDS = ((7, 8), (9, 10))          # rank r's two loader batches


def _w2k2_worker(rank, world, port, path):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from torch.distributed.algorithms.ddp_comm_hooks import default_hooks
    from monosowa_amd.helpers import trainer_helper
    from monosowa_amd.monodetr.criterion import weighted_total
    from monosowa_amd.synthetic import prepare_targets
    model, crit, opt = _build()
    loader = _Loader(W2_SEEDS[rank])
    state = _seed_hook(model)
    trainer = _trainer(model, crit, opt, loader, global_batch=8)
    ddp = trainer.model
    assert isinstance(ddp, torch.nn.parallel.DistributedDataParallel) and trainer.accum_steps == 2
    ddp.train(), crit.train()
    counts = [_count(b) for b in loader.batches]
    every = [torch.zeros(2, dtype=torch.int64) for _ in range(world)]
    dist.all_gather(every, torch.tensor(counts))
    every = [int(c) for t in every for c in t]
    assert every[:2] == [BOXES[7], BOXES[8]] and len(set(every)) > 1, every
    n_bar = max(sum(every) * crit.group_num / 4.0, 1.0)                  # four virtual ranks

    def flat():
        return torch.cat([p.grad.reshape(-1) for p in model.parameters() if p.grad is not None])

    # the four local micro-gradients, each alone, nothing synchronised
    local = []
    for k, (inputs, calibs, targets, _) in enumerate(loader.batches):
        ddp.zero_grad(set_to_none=True)
        tl = prepare_targets(targets, 2)
        state["k"] = k
        with ddp.no_sync():
            weighted_total(crit(ddp(inputs, calibs, tl, targets["img_size"]), tl, num_boxes=n_bar), crit.weight_dict).backward()
        local.append(flat().clone())
    ddp.zero_grad(set_to_none=True)
    gathered = [torch.zeros(2, local[0].numel()) for _ in range(world)]
    dist.all_gather(gathered, torch.stack(local))
    mean = torch.cat(gathered).sum(0) / 4

    rounds, after_first = [], []

    def hook(_, bucket):
        rounds.append(bucket.index())
        return default_hooks.allreduce_hook(None, bucket)
    ddp.register_comm_hook(None, hook)
    stage = trainer_helper.stage_batch

    def spy(raw, device):
        if raw is loader.batches[1]:                       # micro-step 1 begins: .grad holds micro-step 0 alone
            both = [torch.zeros_like(local[0]) for _ in range(world)]
            dist.all_gather(both, flat())
            after_first.append(bool(torch.equal(both[0], both[1])))
        return stage(raw, device)
    trainer_helper.stage_batch = spy
    state["k"] = 0
    trainer.train_cycle(list(loader))
    trainer_helper.stage_batch = stage
    got = flat().clone()
    both = [torch.zeros_like(got) for _ in range(world)]
    dist.all_gather(both, got)
    assert torch.equal(both[0], both[1])                                   # equal across ranks after the cycle
    assert after_first == [False]                                          # ... and not before its last backward
    assert rounds and sorted(rounds) == list(range(len(rounds))), rounds   # every bucket all-reduced exactly once
    err, scale = float((got - mean).abs().max()), float(mean.abs().max())
    assert err <= 1e-4 * scale, (err, scale)
    if rank == 0:
        torch.save(("ok", err / scale, len(rounds)), path)
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_two_micro_batches_equal_four_virtual_ranks(tmp_path):
    status, ratio, buckets = _spawn(_w2k2_worker, tmp_path / "w2k2.pt")
    print("max|cycle - mean of four| / max|mean| = %.3e, %d buckets" % (ratio, buckets))
    assert status == "ok"


# --------------------------------------------------------------------------------------------------- 4. loop shape
def _frozen(opt):
    """lr = 0: the optimizer runs (and counts) but the parameters keep their bits (p - 0 * update)."""
    for group in opt.param_groups:
        group["lr"] = 0.0
    return opt


def test_five_batches_give_three_steps_and_the_tail_is_a_plain_step():
    from monosowa_amd.helpers.trainer_helper import stage_batch
    model, crit, opt = _build()
    loader = _Loader([7, 8, 9, 10, 11])
    state = _seed_hook(model)
    trainer = _trainer(model, crit, _frozen(opt), loader, global_batch=4)
    before = [p.detach().clone() for p in model.parameters()]
    steps, cycles, plain = [], [], []
    opt_step, train_cycle, train_step = opt.step, trainer.train_cycle, trainer.train_step
    opt.step = lambda *a, **k: (steps.append(1), opt_step(*a, **k))[1]
    trainer.train_cycle = lambda raws: (cycles.append([id(r) for r in raws]), train_cycle(raws))[1]
    trainer.train_step = lambda *a, **k: (plain.append(1), train_step(*a, **k))[1]
    trainer.log_interval = 10 ** 9
    state["k"] = 0
    trainer.train_one_epoch(0)
    ids = [id(b) for b in loader.batches]
    assert len(steps) == 3 and cycles == [ids[0:2], ids[2:4], ids[4:5]] and len(plain) == 1
    assert state["k"] == 5
    assert all(torch.equal(a, b) for a, b in zip(before, model.parameters()))
    tail = _named_grads(model)
    state["k"] = 4                                         # the seed of the epoch's fifth forward
    train_step(*stage_batch(loader.batches[4], trainer.device))
    want = _named_grads(model)
    assert set(tail) == set(want) and all(torch.equal(tail[n], want[n]) for n in want)


@pytest.mark.parametrize("global_batch", ["absent", 2])
def test_without_the_key_or_with_k_1_the_loop_is_the_plain_one(global_batch):
    model, crit, opt = _build()
    loader = _Loader([7, 8])
    _seed_hook(model)
    for off in (None, 0):
        assert _trainer(model, crit, opt, loader, global_batch=off).accum_steps == 1
    cfg = {} if global_batch == "absent" else {"global_batch": global_batch}
    trainer = _trainer(model, crit, _frozen(opt), loader, **cfg)
    assert trainer.accum_steps == 1
    calls = []
    train_step = trainer.train_step
    trainer.train_step = lambda *a, **k: (calls.append(1), train_step(*a, **k))[1]

    def never(*a, **k):
        raise AssertionError("the accumulation code was entered")
    trainer.train_cycle = never
    trainer._cycle_num_boxes = never
    trainer.log_interval = 10 ** 9
    trainer.train_one_epoch(0)
    assert len(calls) == 2 and trainer._accumulator is None


def test_global_batch_must_be_a_multiple_of_world_times_batch():
    model, crit, opt = _build()
    with pytest.raises(ValueError) as e:
        _trainer(model, crit, opt, _Loader([], batch_size=4), global_batch=6)
    words = str(e.value).replace("=", " ").replace(",", " ").split()
    assert "6" in words and "1" in words and "4" in words, str(e.value)
    with pytest.raises(ValueError):
        _trainer(model, crit, opt, _Loader([], batch_size=4), global_batch=-4)
