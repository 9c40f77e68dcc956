"""Writes tests/golden/reference_tables.npz: what the reference's text says about the constant tables the package ships and computes, so that
tests/test_reference_tables.py holds them to it on every machine.  Run where the reference tree exists (its path as the argument):

    python tests/golden/make_reference_tables.py <reference>/src/core

  primes, prime_sums     PRIMES / PRIME_SUMS of lowdiscrepancy.rs:20-150 (1000 entries each)
  sobol_sha256           sha256 of what tools/convert_sobol_tables.py writes from sobolmatrices.rs (the bytes of rs_pbrt_amd/data/sobol_tables.bin)
  maxmin_sha256          sha256 of what tools/convert_maxmin_table.py writes from lowdiscrepancy.rs (the bytes of rs_pbrt_amd/data/maxmin_tables.bin)"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))


def prime_table(text, name):
    m = re.search(r"pub const %s: \[u32; PRIME_TABLE_SIZE as usize\] = \[(.*?)\];" % name, text, re.S)
    body = re.sub(r"//.*", "", m.group(1))
    return np.array([int(x.replace("_", "")) for x in re.findall(r"\b[0-9][0-9_]*\b", body)], np.int64)


def converted_sha256(tool, src):
    """sha256 of the blob tools/<tool> writes from the reference source file src"""
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "table.bin")
        subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", tool), src, out])
        return hashlib.sha256(open(out, "rb").read()).hexdigest()


def tables(ref_core):
    text = open(os.path.join(ref_core, "lowdiscrepancy.rs")).read()
    return {"primes": prime_table(text, "PRIMES"), "prime_sums": prime_table(text, "PRIME_SUMS"),
            "sobol_sha256": np.array(converted_sha256("convert_sobol_tables.py", os.path.join(ref_core, "sobolmatrices.rs"))),
            "maxmin_sha256": np.array(converted_sha256("convert_maxmin_table.py", os.path.join(ref_core, "lowdiscrepancy.rs")))}


if __name__ == "__main__":
    np.savez_compressed(os.path.join(HERE, "reference_tables.npz"), **tables(sys.argv[1]))
