"""The mecat2cns program (mecat_amd/bin/mecat2cns) end to end on the GPU against the four runs of the unmodified reference recorded in
tests/golden/cns_cli.npz (technology x input type, -t 1, three partitions): the output file is byte-identical — whole-file SHA-256, every
header line, SHA-256 of every record, the first records in full — with -t 1, with -t 4 and with the host text (MECAT_CNS_HOST_TEXT=1).
Every run is a fresh child process under its own time limit."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

import cns_cli_cases as CC

pytestmark = pytest.mark.gpu
RUNS = [(n, it) for n in ("pacbio", "nanopore") for it in (0, 1)]


def check_output(key, text):
    K = CC.fixture()
    lines = text.split(b"\n")
    assert lines[-1] == b"" and len(lines) % 2 == 1
    recs = [(lines[i], lines[i + 1]) for i in range(0, len(lines) - 1, 2)]
    headers = [h.decode() for h, _ in recs]
    want = [str(h) for h in K[key + "_headers"]]
    if headers != want:
        i = next((i for i, (a, b) in enumerate(zip(headers, want)) if a != b), min(len(headers), len(want)))
        raise AssertionError("%s: %d records, %d recorded; the first differing header is number %d: %r, recorded %r" % (key, len(headers), len(want), i, headers[i: i + 1], want[i: i + 1]))
    sha = [hashlib.sha256(h + b"\n" + s + b"\n").hexdigest() for h, s in recs]
    bad = [i for i, (a, b) in enumerate(zip(sha, K[key + "_record_sha"])) if a != str(b)]
    assert not bad, "%s: record %d (%s) differs from the recording (%d records differ)" % (key, bad[0], headers[bad[0]], len(bad))
    assert text.startswith(str(K[key + "_first"]).encode())
    assert hashlib.sha256(text).hexdigest() == str(K[key + "_sha"])
    assert len(recs) >= 20


@pytest.mark.parametrize("variant", ["t1", "t4", "host_text"])
@pytest.mark.parametrize("name,input_type", RUNS)
def test_recorded_run(tmp_path, name, input_type, variant):
    run = CC.run_inputs(name, input_type, str(tmp_path))
    out = str(tmp_path / "corrected.fasta")
    env = dict(os.environ)
    env.pop("MECAT_CNS_HOST_TEXT", None)
    if variant == "host_text":
        env["MECAT_CNS_HOST_TEXT"] = "1"
    r = subprocess.run([CC.BIN] + CC.argv_of(run, out, threads=4 if variant == "t4" else 1), capture_output=True, env=env, timeout=150)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    err = r.stderr.decode()
    parts = [l.split("\t")[0] for l in open(run["input"] + ".partition_files").read().splitlines()]
    assert len(parts) >= 3 and all("[processing %s] takes " % p in err for p in parts)
    check_output("%s_%s" % (name, ("can", "m4")[input_type]), open(out, "rb").read())


def test_refuses_a_read_of_max_seq_size(tmp_path):
    """a read of 500 000 letters (MAX_SEQ_SIZE) is refused with a message, exit 1 (a read set over the volume limit is not constructible
    at test size: the same path, the other return value)"""
    fa = str(tmp_path / "long.fasta")
    rng = np.random.default_rng(3)
    with open(fa, "wb") as f:
        f.write(b">short\n" + b"ACGT" * 50 + b"\n>long\n" + np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 500000)].tobytes() + b"\n")
    can = str(tmp_path / "empty.can")
    open(can, "wb").close()
    out = str(tmp_path / "out.fasta")
    r = subprocess.run([CC.BIN, "-i", "0", can, fa, out], capture_output=True, timeout=60)
    assert r.returncode == 1 and "read 1 has 500000 letters or more" in r.stderr.decode()
    assert not os.path.exists(out)
