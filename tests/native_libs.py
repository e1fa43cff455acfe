"""tests/conftest.py builds only librnvp_hip.so.  A test module of an add-on library calls ensure_built(its binding
modules) at import, so that the suite passes on a clean checkout in any order and for any selection of files."""
import os
import subprocess


def ensure_built(*bindings):
    for b in bindings:
        if not os.path.exists(b.LIB_PATH):
            subprocess.check_call(["make", "-C", b.LIBRARY.make_dir, "-s"])
