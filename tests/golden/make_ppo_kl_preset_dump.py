#!/usr/bin/env python
"""Record the parameter objects the reference's Mujoco_PPO preset TEXT produces -> tests/golden/ppo_kl_preset.json, in the
manner of make_pg_preset_dump.py: rl_coach/presets/Mujoco_PPO.py is executed unchanged through this package's import
layer (coach_amd.compat), resolve_reference_style is applied, and agent_params / schedule / preset_validation_params are
stored as tests/test_cartpole.py's _dump writes them, with the name of the golden test's level.  Run from the repo root where the reference
tree is present:

    python tests/golden/make_ppo_kl_preset_dump.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), HERE]

from _refstub import REFERENCE_ROOT  # noqa: E402  (the path only: the stubs are not installed here)

NAME = "Mujoco_PPO"
PARTS = ("agent_params", "schedule", "preset_validation_params")


def main():
    from coach_amd.compat import resolve_reference_style
    from test_cartpole import _dump
    from test_preset_dropin import _exec_preset
    with open(os.path.join(REFERENCE_ROOT, "rl_coach", "presets", NAME + ".py")) as f:
        ref = _exec_preset(f.read())["graph_manager"]
    resolve_reference_style(ref.agent_params, ref.env_params)
    # the preset leaves the level to the command line (SingleLevelSelection(mujoco_v2)): the golden test's level
    ref.env_params.level.select(ref.preset_validation_params.reward_test_level)
    out = {NAME: dict({part: _dump(getattr(ref, part)) for part in PARTS}, level_name=ref.env_params.level_name())}
    path = os.path.join(HERE, "ppo_kl_preset.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True, allow_nan=False)
    print("wrote %s" % path)


if __name__ == "__main__":
    main()
