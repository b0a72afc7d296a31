"""GPU suite: results do not depend on what an engine did before, on where the caller's buffers lie, on the run, or on when the
host waits (tests/state_cases.py).  Everything is compared with the first call of a new engine, byte for byte."""
import pytest

import state_cases as sc

pytestmark = pytest.mark.gpu

NAMES = sc.names(gpu=True)


@pytest.fixture(scope="module")
def base(gpu_engine):
    return sc.Baselines(gpu_engine.L, gpu=True)


@pytest.mark.parametrize("name", NAMES)
def test_dirty_workspace(base, name):
    sc.check_dirty_workspace(base, name)


def test_call_order(base):
    sc.check_call_order(base, NAMES)


def test_deferred_by_one(base):
    """Results do not depend on when the host waits: every case is collected only after the next one has been enqueued."""
    sc.check_deferred(base, NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_red_zones(base, name):
    sc.check_red_zones(base, name)


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("name", [c.name for c in sc.CASES if c.gpu_shapes["vec"]])
def test_misaligned_bases(base, name, k):
    sc.check_red_zones(base, name, k)


@pytest.mark.parametrize("name", [c.name for c in sc.CASES if c.stress])
def test_repeatability(gpu_engine, name):
    """Ten runs at (24, 96, 80): a screen for races on the accumulators, not a hunt."""
    sc.check_repeatable(gpu_engine.L, name)
