"""One FlexGMRES job of tests/golden/ij_saved_flexgmres.json through the driver (hypre_amd.ij.launch): the options the
golden file states for the job line, set in code — the command line itself keeps refusing `-solver 60 | 61`.  Run alone
or as the ranks of a torch.distributed.run job; prints the driver's closing lines.

    python tests/flexgmres_worker.py <name of the golden entry>
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


def main():
    from hypre_amd import ij
    case = json.load(open(os.path.join(HERE, "golden", "ij_saved_flexgmres.json")))[sys.argv[1]]
    opt = ij.IJOptions(**{k: (tuple(v) if isinstance(v, list) else v) for k, v in case["options"].items()})
    return ij.launch(ij.check_options(opt))


if __name__ == "__main__":
    raise SystemExit(main())
