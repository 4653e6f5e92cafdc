"""bench.py with the Adam riders of the convolution weight-gradient launch set from the environment — the same-box A/B of
DESIGN §7.3 item 13 (one process per variant, variants alternated by the caller):

    EARLY=0 python tools/ab_adam_riders.py --gpus 1 --steps 20 --warmup 5          # the one-launch Adam step
    R=256 FIRST=1 python tools/ab_adam_riders.py --gpus 1 --steps 20 --warmup 5    # 256 riders dispatched first

EARLY: ClippedPPOAgent.ADAM_UNDER_CONV_DW; R: nn.graph.ADAM_RIDERS; FIRST: nn.graph.ADAM_RIDERS_FIRST.  Everything else is
bench.py's: its arguments, its one JSON line."""
import os
import runpy
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from coach_amd.agents.clipped_ppo_agent import ClippedPPOAgent      # noqa: E402
from coach_amd.nn import graph as G                                 # noqa: E402

ClippedPPOAgent.ADAM_UNDER_CONV_DW = bool(int(os.environ.get("EARLY", "1")))
G.ADAM_RIDERS = int(os.environ.get("R", G.ADAM_RIDERS))
G.ADAM_RIDERS_FIRST = bool(int(os.environ.get("FIRST", "0")))
sys.argv = [os.path.join(ROOT, "bench.py")] + sys.argv[1:]
runpy.run_path(sys.argv[0], run_name="__main__")
