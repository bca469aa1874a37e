"""Writes tests/golden/scaled_mse_n*.npz: the exact-rational linear-scaling
reference (tests/scaled_ref.py) of the GPU suite's population on each of its
case counts — two and a half minutes of gp.compile calls and exact sums.

    python tests/golden/_ref_scaled_mse.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import scaled_ref  # noqa: E402

if __name__ == "__main__":
    scaled_ref.write_golden()
