"""Classes per block of the slice form's class storage for one operator: the histogram and the sizes of the three arrays.

    python tools/slice_class_stats.py [n] [--problem laplacian|27pt|difconv] [--aniso]
"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hypre_amd import binding as B, ij   # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("n", type=int, nargs="?", default=256)
ap.add_argument("--problem", default="laplacian")
ap.add_argument("--aniso", action="store_true", help="difconv with diffusion coefficients 1, 0.1, 0.01")
args = ap.parse_args()
L = B.load_library()
opt = ij.IJOptions(n=(args.n,) * 3, problem=args.problem)
if args.aniso:
    opt.c = (1.0, 0.1, 0.01)
A = ij.build_matrix(opt)
L.hypre_ParCSRMatrixMigrate(A, B.HYPRE_MEMORY_DEVICE)
diag = A.contents.diag
hist, blocks, total = (C.c_int * 256)(), C.c_int(), C.c_longlong()
most = L.hypre_amd_CSRMatrixPlanSliceClassHistogram(diag, hist, C.byref(blocks), C.byref(total))
B.check()
lanes = L.hypre_amd_CSRMatrixPlanSliceForm(diag)
kp = 8 if lanes == 1 else 16
print(json.dumps({"problem": args.problem + (" aniso" if args.aniso else ""), "n": args.n, "form": L.hypre_amd_CSRMatrixPlanForm(diag),
                  "lanes_per_row": lanes, "most_classes": most, "blocks": blocks.value, "classes_total": total.value,
                  "histogram": {str(c): hist[c] for c in range(256) if hist[c]},
                  "bytes": {"d_sl_cls": 256 * blocks.value, "d_sl_tab": 4 * kp * total.value, "d_sl_toff": 4 * (blocks.value + 1),
                            "packed_words_replaced": blocks.value * 256 * 3 * kp}}))
