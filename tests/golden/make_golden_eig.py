"""Writes tests/golden/eig_yardstick.json: (resid, orth, eigs, sweeps) of the NumPy transcription tests/eig_cases.jacobi
on every input of tests/test_eig_gpu.py.  Run from the repository root: python tests/golden/make_golden_eig.py"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from tests import eig_cases as ec  # noqa: E402

CASES = [('indef', n) for n in (1, 2, 3, 6, 63, 64, 130)] + [(kind, n) for n in (65, 257) for kind in ec.KINDS]


def main():
  out = {}
  for dtype in (np.float32, np.float64):
    for kind, n in CASES:
      out[ec.key(kind, n, dtype)] = list(ec.yardstick(kind, n, dtype, live=True))
      print(ec.key(kind, n, dtype), out[ec.key(kind, n, dtype)], flush=True)
  with open(ec.GOLDEN, 'w') as f:
    json.dump(out, f, indent=1, sort_keys=True)
    f.write('\n')


if __name__ == '__main__':
  main()
