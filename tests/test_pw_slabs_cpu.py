"""SlabQueue and the stage clocks (mecat_amd/host/pw_slabs.h: the two slab buffers of the mecat2pw driver and their hand-over to the
writer thread) under ThreadSanitizer: tests/pw_slabs_check.cpp, a stand-alone program with stub buffers and no library, over rows of
1, 2, 1 + 1 + 5 and 3 + 0 + 2 slabs, with and without the drain after a cell.  CPU only.

The program runs with address-space randomisation off (`setarch -R`, a setting of that one process): the ThreadSanitizer runtime of
gcc 11 supports the program and its libraries only where 28-bit mmap randomisation puts them, and dies at start, before main, on a host
that spreads them wider."""
import os
import platform
import subprocess


def test_slab_queue_under_thread_sanitizer(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "pw_slabs_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-pthread", "-fsanitize=thread", "-I" + os.path.join(root, "include"),
                    "-I" + os.path.join(root, "mecat_amd", "host"), os.path.join(root, "tests", "pw_slabs_check.cpp"), "-o", exe], check=True)
    r = subprocess.run(["setarch", platform.machine(), "-R", exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    out, err = r.stdout.decode(), r.stderr.decode()
    assert r.returncode == 0, err[-2000:]
    assert "8 rows" in out and "ThreadSanitizer" not in err, err[-2000:]
