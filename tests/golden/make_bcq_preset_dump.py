#!/usr/bin/env python
"""Record the parameter objects the reference's CartPole_DDQN_BCQ_BatchRL preset TEXT produces ->
tests/golden/bcq_preset.json, in the manner of make_pal_preset_dump.py: rl_coach/presets/CartPole_DDQN_BCQ_BatchRL.py is
executed unchanged through this package's import layer (coach_amd.compat), resolve_reference_style is applied to both
agents, and the parts of the graph manager are stored as tests/test_cartpole.py's _dump writes them.  Run from the repo
root where the reference tree is present (make_golden_bcq.py runs it as its last step):

    python tests/golden/make_bcq_preset_dump.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), HERE]

from _refstub import REFERENCE_ROOT  # noqa: E402  (the path only: the stubs are not installed here)

NAME = "CartPole_DDQN_BCQ_BatchRL"
PARTS = ("agent_params", "schedule", "preset_validation_params", "experience_generating_agent_params",
         "experience_generating_schedule_params", "visualization_parameters")


def dump_manager(gm):
    from coach_amd.compat import resolve_reference_style
    from test_cartpole import _dump
    resolve_reference_style(gm.agent_params, gm.env_params)
    gm.experience_generating_agent_params.input_filter = getattr(gm.agent_params, "input_filter", None)
    resolve_reference_style(gm.experience_generating_agent_params, gm.env_params)
    out = {part: _dump(getattr(gm, part)) for part in PARTS}
    ep = gm.env_params                     # (the device CartPole's own parameters carry the level as a field)
    out["level_name"] = ep.level_name() if hasattr(ep, "level_name") else ep.level
    out["reward_model_num_epochs"] = gm.reward_model_num_epochs
    out["is_collecting_random_dataset"] = gm.is_collecting_random_dataset
    return out


def main():
    from test_preset_dropin import _exec_preset
    with open(os.path.join(REFERENCE_ROOT, "rl_coach", "presets", NAME + ".py")) as f:
        gm = _exec_preset(f.read())["graph_manager"]
    path = os.path.join(HERE, "bcq_preset.json")
    with open(path, "w") as f:
        json.dump({NAME: dump_manager(gm)}, f, indent=1, sort_keys=True, allow_nan=False)
    print("wrote %s" % path)


if __name__ == "__main__":
    main()
