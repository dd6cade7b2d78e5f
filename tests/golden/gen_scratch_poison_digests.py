"""Writes tests/golden/scratch_poison_cdict_digests.json (needs the GPU and the debug-hook library): the digests of the frames a digested
formatted dictionary gives for the batch of tests/_poison.py - _usingCDict and the CDict set, levels 1, 3 and 4.  It runs the whole
family (tests/_poison.py family_compress_dict: every frame passes its oracle D round trip, every run of a case on fresh, filled and
prefilled memory must give the same frames) with the digest check replaced by a recorder."""
import json, os, sys
os.environ["ZSMI_DEBUG_LIB"] = "1"
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import _cdict as K
import _poison as P

seen = {}
P.check_digest = lambda name, got, what: seen.setdefault(name, set()).add(K.frames_digest([f for _, f in got]))
P.family_compress_dict()
assert all(len(v) == 1 for v in seen.values()), seen
json.dump({k: next(iter(v)) for k, v in sorted(seen.items())}, open(P.DIGESTS, "w"), indent=1)
print("wrote", P.DIGESTS, len(seen))
