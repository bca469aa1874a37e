"""Writes tests/golden/abs_error_n*.npz: the Python reference of
``SymbRegAbsError`` (tests/abs_error_ref.py) of the GPU suite's population on
each of its case counts — two minutes of gp.compile calls.

    python tests/golden/_ref_abs_error.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import abs_error_ref  # noqa: E402

if __name__ == "__main__":
    abs_error_ref.write_golden()
