#!/bin/bash
# Development aid: builds kernel-shape variants of the library as zstandard_amd/lib/var_<name>.so (they travel to the GPU box);
# usage: tools/build_variants.sh name1:"-DX=1 -DY=2" name2:"..."   (tools/variants.sh runs them there; tools/README.md)
# The compile command is zstandard_amd/_lib.py's own: ZSMI_LIB_FILE names the output, ZSMI_HIPCC_FLAGS the variant's flags (part of its fingerprint).
rm -f zstandard_amd/lib/var_*.so
for spec in "$@"; do
    name=${spec%%:*}; flags=${spec#*:}
    ZSMI_LIB_FILE=$PWD/zstandard_amd/lib/var_${name}.so ZSMI_HIPCC_FLAGS="$flags" python3 -c "from zstandard_amd import _lib; _lib.build(force=True)" 2>&1 | grep -v 'warning: argument unused' &
    if (( $(jobs -r | wc -l) >= 4 )); then wait -n; fi
done
wait
ls -la zstandard_amd/lib/var_*.so
