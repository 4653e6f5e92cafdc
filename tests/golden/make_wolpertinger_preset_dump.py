#!/usr/bin/env python
"""Record the parameter objects the reference's Mujoco_Wolpertinger preset TEXT produces ->
tests/golden/wolpertinger_preset.json, in the manner of make_rainbow_preset_dump.py: the text is executed unchanged
through this package's import layer (coach_amd.compat), resolve_reference_style is applied, and agent_params / env_params /
schedule / preset_validation_params are stored as tests/test_cartpole.py's _dump writes them, plus the output filter's
contents (which _dump, skipping private fields, does not reach).  Run from the repo root where the reference tree is
present:

    python tests/golden/make_wolpertinger_preset_dump.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), HERE]

from _refstub import REFERENCE_ROOT  # noqa: E402  (the path only: the stubs are not installed here)

NAME = "Mujoco_Wolpertinger"
PARTS = ("agent_params", "env_params", "schedule", "preset_validation_params")


def main():
    from coach_amd.compat import resolve_reference_style
    from test_cartpole import _dump
    from test_preset_dropin import _exec_preset
    with open(os.path.join(REFERENCE_ROOT, "rl_coach", "presets", NAME + ".py")) as f:
        ref = _exec_preset(f.read())["graph_manager"]
    resolve_reference_style(ref.agent_params, ref.env_params)
    out = {NAME: {part: _dump(getattr(ref, part)) for part in PARTS}}
    filters = ref.agent_params.output_filter.action_filters
    out[NAME]["action_filters"] = {name: _dump(f) for name, f in filters.items()}
    path = os.path.join(HERE, "wolpertinger_preset.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True, allow_nan=False)
    print("wrote %s" % path)


if __name__ == "__main__":
    main()
