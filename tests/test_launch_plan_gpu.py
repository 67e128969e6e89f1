"""The launch list of the forward and training schedules, launch by launch: every configuration of tests/golden/launch_plan.json (recorded by
tests/tools/gen_launch_plan.py before the schedules' kernel choice moved into cerberus_amd/csrc/conv_plan.h) is replayed and must produce the same
(layer name, kernel family) sequence, the same flops per record and the same NetDesc.flops(n, h, w)."""
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import gen_launch_plan  # noqa: E402

PLAN = gen_launch_plan.load_plan()


def test_plan_file_covers_every_configuration():
    assert [c["id"] for c in gen_launch_plan.configs()] == list(PLAN)
    for cfg in gen_launch_plan.configs():
        assert PLAN[cfg["id"]][0] == cfg
    assert os.path.getsize(gen_launch_plan.PLAN) < 1 << 20


@pytest.fixture(scope="module")
def state_dict():
    import torch

    from cerberus_amd.weights import make_state_dict

    return {k: torch.from_numpy(v) for k, v in make_state_dict(gen_launch_plan.SEED).items()}


@pytest.mark.gpu
@pytest.mark.parametrize("cid", list(PLAN))
def test_schedule_replays_the_recorded_launch_plan(cid, state_dict):
    cfg, want, want_flops = PLAN[cid]
    got, got_flops = gen_launch_plan.run_config(cfg, state_dict)
    assert [(r[0], r[1]) for r in got] == [(r[0], r[1]) for r in want]
    bad = [(g[0], g[1], g[2], w[2]) for g, w in zip(got, want) if g[2] != w[2]]
    assert not bad, bad[:5]
    assert got_flops == want_flops
