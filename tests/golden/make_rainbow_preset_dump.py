#!/usr/bin/env python
"""Record the parameter objects the reference's CartPole_Rainbow and Atari_Rainbow preset TEXTS produce ->
tests/golden/rainbow_preset.json, in the manner of make_c51_preset_dump.py: each text is executed unchanged through this
package's import layer (coach_amd.compat), resolve_reference_style is applied, and agent_params / env_params / schedule /
preset_validation_params are stored as tests/test_cartpole.py's _dump writes them.  Run from the repo root where the
reference tree is present:

    python tests/golden/make_rainbow_preset_dump.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), HERE]

from _refstub import REFERENCE_ROOT  # noqa: E402  (the path only: the stubs are not installed here)

NAMES = ("CartPole_Rainbow", "Atari_Rainbow")
PARTS = ("agent_params", "env_params", "schedule", "preset_validation_params")


def main():
    from coach_amd.compat import resolve_reference_style
    from test_cartpole import _dump
    from test_preset_dropin import _exec_preset
    out = {}
    for name in NAMES:
        with open(os.path.join(REFERENCE_ROOT, "rl_coach", "presets", name + ".py")) as f:
            ref = _exec_preset(f.read())["graph_manager"]
        resolve_reference_style(ref.agent_params, ref.env_params)
        out[name] = {part: _dump(getattr(ref, part)) for part in PARTS}
    path = os.path.join(HERE, "rainbow_preset.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True, allow_nan=False)
    print("wrote %s" % path)


if __name__ == "__main__":
    main()
