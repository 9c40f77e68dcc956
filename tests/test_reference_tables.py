"""The constant tables the package ships (rs_pbrt_amd/data/*.bin) and computes (the Halton primes) held to the reference's text (round 6, VERDICT r5 next #4a).
tests/golden/reference_tables.npz (tests/golden/make_reference_tables.py) carries what the text gives: PRIMES / PRIME_SUMS (lowdiscrepancy.rs:20-150) and the
sha256 of what tools/convert_sobol_tables.py / convert_maxmin_table.py write from src/core/{sobolmatrices,lowdiscrepancy}.rs.  The committed blobs and
scenes.first_primes are held to that fixture everywhere; where the reference tree exists the converters are re-run on it as well, and the fixture is held to it."""
import hashlib
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = "/root/reference/src/core/"
HAVE_REF = os.path.exists(REF + "sobolmatrices.rs")
G = np.load(os.path.join(HERE, "golden", "reference_tables.npz"))


@pytest.mark.parametrize("tool,src,blob", [("convert_sobol_tables.py", "sobolmatrices.rs", "sobol_tables.bin"), ("convert_maxmin_table.py", "lowdiscrepancy.rs", "maxmin_tables.bin")])
def test_committed_table_is_the_references(tool, src, blob):
    key = blob.replace("_tables.bin", "_sha256")
    committed = open(os.path.join(ROOT, "rs_pbrt_amd", "data", blob), "rb").read()
    assert hashlib.sha256(committed).hexdigest() == str(G[key]), "%s differs from what %s gives (tests/golden/reference_tables.npz)" % (blob, src)
    if HAVE_REF:
        from tests.golden.make_reference_tables import converted_sha256
        assert converted_sha256(tool, REF + src) == str(G[key]), "tests/golden/reference_tables.npz is stale against %s" % src


def test_halton_primes_and_their_sums_are_the_references():
    from rs_pbrt_amd import scenes
    primes, sums = G["primes"], G["prime_sums"]
    assert len(primes) == 1000 and len(sums) == 1000
    mine = np.array(scenes.first_primes(1000), np.int64)
    assert np.array_equal(mine, primes)
    assert np.array_equal(np.concatenate([[0], np.cumsum(mine)[:-1]]), sums)      # PRIME_SUMS[i] = sum of the primes before i
    if HAVE_REF:
        from tests.golden.make_reference_tables import prime_table
        text = open(REF + "lowdiscrepancy.rs").read()
        assert np.array_equal(prime_table(text, "PRIMES"), primes) and np.array_equal(prime_table(text, "PRIME_SUMS"), sums), "tests/golden/reference_tables.npz is stale"
