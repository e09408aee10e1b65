"""aln_jobs_check (mecat_amd/csrc/aln_jobs.h: the one check of a host job list that mhip_align_candidates and mhip_xalign_candidates
share): tests/aln_jobs_check.cpp, a stand-alone program on two reads of 20 and 30 bases with one case per rule, each at every place of
a list of three, built with the sanitizers' runtime linked in.  CPU only."""
import os
import subprocess


def test_job_check_rules(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "aln_jobs_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(root, "mecat_amd", "csrc"), "-I" + os.path.join(root, "include"),
                    os.path.join(root, "tests", "aln_jobs_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    out, err = r.stdout.decode(), r.stderr.decode()
    print(out)
    assert r.returncode == 0, out + err[-2000:]
    assert "aln_jobs_check: 0 wrong" in out and "WRONG" not in out and "Sanitizer" not in err and "runtime error" not in err, out + err[-2000:]
    # the messages, character for character those of the two entry points before they shared the check
    assert "qstart == size + 1           at 1: refused: alignment job 1: start point outside the reads\n" in out
    assert "sid_local == num_reads       at 2: refused: alignment job 2: read index out of range\n" in out
    assert out.count("accepted") == 9 and out.count("refused: ") == 15
