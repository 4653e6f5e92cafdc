#!/usr/bin/env python
"""Record the parameter objects the reference's CartPole preset TEXTS produce -> tests/golden/cartpole_presets.json.

Each rl_coach/presets/<name>.py is executed unchanged through this package's import layer (coach_amd.compat, as
tests/test_preset_dropin.py does), resolve_reference_style is applied, and agent_params / schedule /
preset_validation_params are stored as tests/test_cartpole.py's _dump writes them.  The test compares the package's
own coach_amd/presets/<name>.py against this record.  Run from the repo root where the reference tree is present
(its location as in _refstub.py):

    python tests/golden/make_preset_dumps.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), HERE]

from _refstub import REFERENCE_ROOT  # noqa: E402  (the path only: the stubs are not installed here)

NAMES = ("CartPole_DQN", "CartPole_ClippedPPO")
PARTS = ("agent_params", "schedule", "preset_validation_params")


def main():
    from coach_amd.compat import resolve_reference_style
    from test_cartpole import _dump
    from test_preset_dropin import _exec_preset
    out = {}
    for name in NAMES:
        with open(os.path.join(REFERENCE_ROOT, "rl_coach", "presets", name + ".py")) as f:
            ref = _exec_preset(f.read())["graph_manager"]
        resolve_reference_style(ref.agent_params, ref.env_params)
        out[name] = {"level_name": ref.env_params.level_name()}
        for part in PARTS:
            out[name][part] = _dump(getattr(ref, part))
    path = os.path.join(HERE, "cartpole_presets.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True, allow_nan=False)
    print("wrote %s" % path)


if __name__ == "__main__":
    main()
