#!/usr/bin/env python3
"""Regenerate tests/golden/reentry_files/{eclipse,transit}/: the files the reference's own library
interface leaves behind after the three runs of reentry_inputs.txt (run_transit writes them on
every call, do_transit transit.c:125-207, so these are the third run's).

Run in the build container only: oracle/_ref/transit_reentry (oracle/ref_reentry_main.c around the
compiled reference, built by `make -C oracle ref`) runs in a scratch copy of tests/golden/reentry
and tests/golden/reentry_transit.  Only the output files are kept.

    python tests/golden/reentry_files/make_files.py
"""
import os
import shutil
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.dirname(HERE)
ROOT = os.path.dirname(os.path.dirname(GOLDEN))
REF_REENTRY = os.path.join(ROOT, "oracle", "_ref", "transit_reentry")

CASES = {"eclipse": "reentry", "transit": "reentry_transit"}
FILES = ("spectrum.dat", "toomuch.dat", "tau.dat", "CIA.dat", "mol_extion.dat")


def main():
    for name, case in CASES.items():
        with tempfile.TemporaryDirectory() as tmp:
            work = os.path.join(tmp, case)
            shutil.copytree(os.path.join(GOLDEN, case), work)
            for f in FILES:
                if os.path.exists(os.path.join(work, f)):
                    os.remove(os.path.join(work, f))
            subprocess.run([REF_REENTRY, "case.cfg", "reentry_inputs.txt", "ref_out"], cwd=work, check=True,
                           stdout=subprocess.DEVNULL, timeout=600)
            dest = os.path.join(HERE, name)
            os.makedirs(dest, exist_ok=True)
            for f in FILES:
                shutil.copy(os.path.join(work, f), os.path.join(dest, f))
            print(name, "->", dest)


if __name__ == "__main__":
    main()
