"""tests/ranks.py itself, over gloo on the CPU: what run_ranks returns, and that no rank outlives it when one of them
raises, exits hard or overruns the limit.  Only that it returns and that the children are gone is asserted, no wall time."""
import multiprocessing
import os
import time

import pytest

from tests.ranks import run_ranks


def _sum_ranks(rank, world):
    import torch
    import torch.distributed as dist
    t = torch.tensor([rank + 1.0])
    dist.all_reduce(t)
    assert t.item() == world * (world + 1) / 2
    return rank * 10


def _one_raises(rank, world):
    import torch.distributed as dist
    if rank == 1:
        raise ValueError("boom")
    dist.barrier()


def _one_exits(rank, world):
    import torch.distributed as dist
    if rank == 1:
        os._exit(7)
    dist.barrier()


def _one_sleeps(rank, world):
    if rank == 0:
        time.sleep(60)


def test_both_ranks_succeed():
    assert run_ranks(_sum_ranks, 2, timeout=120) == [0, 10]
    assert multiprocessing.active_children() == []


def test_one_rank_raises():
    with pytest.raises(AssertionError) as e:
        run_ranks(_one_raises, 2, timeout=120, grace=2)
    text = str(e.value)
    assert "boom" in text and "ValueError" in text.split("rank 1:")[1] and "ValueError" not in text.split("rank 1:")[0]
    assert multiprocessing.active_children() == []


def test_one_rank_exits_hard():
    with pytest.raises(AssertionError) as e:
        run_ranks(_one_exits, 2, timeout=120, grace=2)
    assert "rank 1: exit code 7" in str(e.value)
    assert multiprocessing.active_children() == []


def test_one_rank_overruns():
    with pytest.raises(AssertionError) as e:
        run_ranks(_one_sleeps, 2, timeout=3)
    assert "rank 0: killed at the 3 s limit" in str(e.value) and "rank 1: ok" in str(e.value)
    assert multiprocessing.active_children() == []


def test_a_function_that_cannot_be_pickled_fails_in_the_parent():
    with pytest.raises(Exception) as e:
        run_ranks(lambda rank, world: None, 2, timeout=120)
    assert not isinstance(e.value, AssertionError) and "pickle" in (type(e.value).__name__ + str(e.value)).lower()
    assert multiprocessing.active_children() == []
