"""The dm_host.o rule of both Makefiles (deepmimic_amd/csrc, tests/emu) rebuilds the object when any header dm_host.cpp includes changes: an emulator library
left standing on an old object would let the CPU suite pass against code that is no longer in the tree.  Dry runs only: no compiler, no GPU."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "deepmimic_amd", "csrc")
MAKEFILES = {"product": (CSRC, ""), "emulator": (os.path.join(ROOT, "tests", "emu"), "../../deepmimic_amd/csrc/")}      # directory, how its rules spell csrc/


def included_headers():
    return sorted(set(re.findall(r'^\s*#\s*include\s+"(dm_\w+\.h)"', open(os.path.join(CSRC, "dm_host.cpp")).read(), re.M)))


def compiles_dm_host(mk_dir, objdir, *flags):
    """does a dry run for <objdir>/dm_host.o print a command that compiles dm_host.cpp?"""
    out = subprocess.run(["make", "-C", mk_dir, "-n", *flags, "OBJDIR=%s" % objdir, "%s/dm_host.o" % objdir], check=True, capture_output=True, text=True).stdout
    return any(re.search(r"\s-c\s", l) and "dm_host.cpp" in l for l in out.splitlines())


@pytest.mark.parametrize("which", sorted(MAKEFILES))
def test_dm_host_object_depends_on_every_header_it_includes(which, tmp_path):
    mk_dir, prefix = MAKEFILES[which]
    headers = included_headers()
    assert {"dm_norm.h", "dm_returns.h", "dm_ppo_batch.h", "dm_replay.h"} <= set(headers)
    (tmp_path / "dm_host.o").write_bytes(b"")           # an object newer than every source: up to date unless a prerequisite counts as changed
    assert not compiles_dm_host(mk_dir, str(tmp_path))
    for h in headers:
        assert compiles_dm_host(mk_dir, str(tmp_path), "-W", prefix + h), "%s Makefile: a change of %s does not rebuild dm_host.o" % (which, h)
