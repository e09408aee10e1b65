"""concat_slices and parallel_memcpy (mecat_amd/csrc/cns_slices.h: how the accept stage puts its slices' variable-length outputs
together) under AddressSanitizer and UndefinedBehaviorSanitizer: tests/cns_slices_check.cpp, a stand-alone program with the sanitizers'
runtime linked in, over a few thousand seeded random slice sets against a naive concatenation.  CPU only."""
import os
import subprocess


def test_concat_slices_under_sanitizers(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "cns_slices_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(root, "mecat_amd", "csrc"), os.path.join(root, "tests", "cns_slices_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    out, err = r.stdout.decode(), r.stderr.decode()
    assert r.returncode == 0, err[-2000:]
    assert "4000 slice sets" in out and "Sanitizer" not in err and "runtime error" not in err, err[-2000:]
