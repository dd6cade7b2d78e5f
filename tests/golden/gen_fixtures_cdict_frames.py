#!/usr/bin/env python3
"""Generates tests/golden/cdict_frame_digests.json: the SHA-256 of the frames a CompressionDict of each formatted dictionary of
tests/_cdict.py pin_cases() writes for its records, at levels 1 and 3 (entry <dictionary>_l<level>; digest: _cdict.frames_digest).  No
oracle writes Repeat_Mode or treeless blocks, so the library's own frames at the commit that introduced the pin are the record: run it
only to add cases, at a commit whose frames are trusted, never to make a failing test pass.  Needs the GPU.
Run from the repo root: python tests/golden/gen_fixtures_cdict_frames.py [output file]"""
import json, os, sys
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE)); sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import _cdict as K
import _batch as B
from zstandard_amd import BatchCodec, CompressionDict

codec = BatchCodec(0)
out = {}
for name, (dic, records) in K.pin_cases().items():
    for level in K.PIN_LEVELS:
        cd = CompressionDict(codec, dic, level)
        frames = B.compress_many(codec, records, cdict=cd)
        cd.close()
        B.assert_round_trip(codec, frames, records, dic, name)
        first = [K.blocks_of(f)[0] for f in frames]
        print(name, level, "treeless", sum(b[1] == 3 for b in first), "repeat", sum(K.uses_repeat_mode(b) for b in first), "of", len(frames))
        out[f"{name}_l{level}"] = K.frames_digest(frames)
path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "cdict_frame_digests.json")
with open(path, "w") as f:
    json.dump(out, f, indent=0, sort_keys=True)
    f.write("\n")
print("wrote", path)
