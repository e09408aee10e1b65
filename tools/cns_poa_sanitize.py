#!/usr/bin/env python3
"""The POA window routine (mecat_amd/csrc/cns_poa.h) under AddressSanitizer and UndefinedBehaviorSanitizer, on the CPU: writes the
cases of tests/golden/cns_poa.npz with their pieces and recorded strings as a packed case file, builds mecat_amd/csrc/cns_poa_host.cpp
with -DCNS_POA_MAIN -fsanitize=address,undefined as a stand-alone program and runs it over the file.  The program exits non-zero when a
window differs from its recorded string; the sanitizers abort on the first finding.
    python tools/cns_poa_sanitize.py"""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cns_poa_cases as P  # noqa: E402


def main():
    cases, strings = P.load_fixture()
    tails = [P.pieces_of(c) + (row,) for c, row in zip(cases, strings)]
    with tempfile.TemporaryDirectory() as tmp:
        data, exe = os.path.join(tmp, "cases.bin"), os.path.join(tmp, "cns_poa_check")
        P.write_cases(data, cases, tails)
        src = os.path.join(ROOT, "mecat_amd", "csrc")
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DCNS_POA_MAIN", "-I" + src,
                        os.path.join(src, "cns_poa_host.cpp"), "-o", exe], check=True)
        return subprocess.run([exe, data]).returncode


if __name__ == "__main__":
    sys.exit(main())
