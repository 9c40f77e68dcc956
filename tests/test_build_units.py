"""CPU: the instantiation groups that tu_decl.h declares are the groups the Makefile builds (one compile of tu.hip each), and
csrc/ holds no other unit source.  A group declared but not built is a link error (-Wl,--no-undefined); this names it sooner."""
import glob
import os
import re
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rs_pbrt_amd", "csrc")


@pytest.mark.skipif(shutil.which("make") is None, reason="make is not installed")
def test_declared_groups_are_the_built_groups():
    declared = set(re.findall(r"\bRSPT_TU_GROUP_([A-Z0-9_]+)", open(os.path.join(CSRC, "tu_decl.h")).read()))
    built = subprocess.run(["make", "-s", "--no-print-directory", "-C", CSRC, "groups"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True, check=True).stdout.split()
    assert len(built) == len(set(built)), sorted(g for g in set(built) if built.count(g) > 1)
    assert set(built) == declared, (sorted(declared - set(built)), sorted(set(built) - declared))
    assert sorted(os.path.basename(f) for f in glob.glob(os.path.join(CSRC, "*.hip"))) == ["librspt.hip", "tu.hip"]
