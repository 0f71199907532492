"""``python -m manner_amd.run <script.py> [args…]`` — run one of the reference's entry points (manner/train.py, manner/eval.py)
with the HIP operator classes installed, without editing a line of the reference:

    cd <checkout of andreeaiana/manner>
    PYTHONPATH=<this repository> python -m manner_amd.run manner/train.py experiment=cr_module_mind_title_scl_lf

``--baselines NAME[,NAME...]`` in front of the script path opts into further mirrored classes (``install(baselines=...)``):

    PYTHONPATH=<this repository> python -m manner_amd.run --baselines miner manner/train.py experiment=miner_weighted_mind
    PYTHONPATH=<this repository> python -m manner_amd.run --baselines caum_plm manner/train.py experiment=caum_plm_mind
    PYTHONPATH=<this repository> python -m manner_amd.run --baselines lstur_plm manner/train.py experiment=lstur_ini_mind
    PYTHONPATH=<this repository> python -m manner_amd.run --baselines mins_plm manner/train.py experiment=mins_mind

``install()`` runs first (manner_amd/binding.py), then the script runs as ``__main__`` with ``sys.argv`` shifted, exactly as
``python <script.py> [args…]`` would (the script's directory is put first on ``sys.path`` as the interpreter does; the current
directory is added so that ``import manner`` finds the checkout — the reference's own scripts rely on ``pyrootutils`` for that,
reference manner/train.py:11)."""
from __future__ import annotations

import os
import runpy
import sys


def main() -> None:
    usage = "usage: python -m manner_amd.run [--baselines NAME[,NAME...]] <script.py> [args...]"
    baselines = ()
    if len(sys.argv) > 1 and (sys.argv[1] == "--baselines" or sys.argv[1].startswith("--baselines=")):
        if "=" in sys.argv[1]:
            value = sys.argv.pop(1).split("=", 1)[1]
        else:
            if len(sys.argv) < 3:
                raise SystemExit(usage)
            del sys.argv[1]
            value = sys.argv.pop(1)
        baselines = tuple(b for b in value.split(",") if b)
    if len(sys.argv) < 2:
        raise SystemExit(usage)
    script = os.path.abspath(sys.argv[1])
    cwd = os.getcwd()
    if cwd not in sys.path:
        sys.path.insert(0, cwd)
    from manner_amd.binding import install
    rebound = install(baselines=baselines)
    print("[manner_amd] installed: " + "; ".join(f"{m.rsplit('.', 1)[1]}: {', '.join(v)}" for m, v in rebound.items()), file=sys.stderr)
    sys.argv = [script] + sys.argv[2:]
    sys.path.insert(0, os.path.dirname(script))
    runpy.run_path(script, run_name="__main__")


if __name__ == "__main__":
    main()
