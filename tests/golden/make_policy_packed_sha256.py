#!/usr/bin/env python
"""Golden hashes of the packed policy arrays: tests/golden/policy_packed_sha256.json.

The committed file was made from commit f6a6f35 ("Add scalar heads to the device nets: critic value, AMP style reward"), the last one whose
dm_policy_create(_gated) packed its weights on the host (three scalar packers in dm_policy_host.h, docs/HISTORY.md section 15): its emulator build
(make -C tests/emu) created one context per case of tests/test_policy_set_weights.py GOLDEN_CASES -- every entry of SHAPES, with and without the optional
arrays -- from golden_weights (integer arithmetic only, the SPECIAL bit patterns planted in every matrix), and every array the context holds was read back
with dm_policy_read_packed.  Only sizes and SHA-256 are stored.  Since then create packs with k_policy_pack, and this file is what holds that kernel, and
the numpy statement of the layout in the test, to the bytes the host packers wrote.

Running this script on a later commit records that commit's bytes: do so only when the layout is meant to change, and say from which commit in `commit`.
Usage: python tests/golden/make_policy_packed_sha256.py <commit the library was built from> [path of libdm_emu.so]"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ["DM_ALLOW_EMULATOR"] = "1"

import test_policy_set_weights as t                  # noqa: E402
from deepmimic_amd.policy import Policy              # noqa: E402

if len(sys.argv) < 2:
    raise SystemExit(__doc__)
lib = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "emu", "libdm_emu.so")
cases = {}
for case in t.GOLDEN_CASES:
    pol = Policy(t.golden_weights(case), lib_path=lib, s_clip=t.S_CLIP)
    cases[case] = t.digest(t.packed(pol))
    pol.close()
out = dict(what="size and SHA-256 of dm_policy_read_packed of every array of a context created from test_policy_set_weights.golden_weights(case)",
           commit=sys.argv[1], cases=cases)
with open(os.path.join(HERE, "policy_packed_sha256.json"), "w") as fh:
    json.dump(out, fh, indent=1, sort_keys=True)
    fh.write("\n")
print("wrote %d cases, %d arrays" % (len(cases), sum(len(c) for c in cases.values())))
