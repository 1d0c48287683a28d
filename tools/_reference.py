"""What the gen_golden_* tools share: importing modules of the reference checkout.  Development machine only (the checkout never enters
this repository and never travels to the GPU box)."""
from __future__ import annotations

import importlib
import os
import sys


def import_reference(ref, *names):
    """The genuine reference modules `names`, imported from the checkout at `ref`."""
    if not os.path.isdir(ref):
        sys.exit(f"reference checkout not found at {ref}; golden vectors can only be regenerated on the development machine")
    sys.path.insert(0, ref)
    os.environ.setdefault("MPLBACKEND", "Agg")
    cwd = os.getcwd()
    os.chdir("/tmp")                        # (the reference's modules write nothing, but they import from the working directory first)
    try:
        return [importlib.import_module(n) for n in names]
    finally:
        os.chdir(cwd)
