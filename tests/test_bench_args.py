"""bench.py's switches, without a GPU: a plain run leaves every leg that takes runs of its own to --full."""
import pytest

import bench


def test_plain_run_is_not_full():
    assert not bench.parse_args(["--gpus", "1", "--steps", "5", "--warmup", "2"]).full
    assert bench.parse_args(["--gpus", "1", "--steps", "5", "--warmup", "2", "--full"]).full


def test_force_weak_leg_needs_full():
    with pytest.raises(SystemExit):
        bench.parse_args(["--force-weak-leg"])
    assert bench.parse_args(["--full", "--force-weak-leg"]).force_weak_leg
