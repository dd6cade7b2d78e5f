#!/bin/bash
# Development aid (GPU box): runs every kernel-shape variant built as zstandard_amd/lib/var_<name>.so (tools/build_variants.sh name:"-DX=n" ...).
# usage: tools/variants.sh bench | l1 | kernels | decode [bench_decode.py flags, e.g. --libzstd] | check NAME | checkdec NAME   (tools/README.md)
# Every step runs under its own timeout; the first step that fails ends the script.
mode=$1; shift
bench() {   # bench line of every variant: value, ratio, per-kernel times
    for f in zstandard_amd/lib/var_*.so; do
        ZSMI_LIB_FILE=$PWD/$f timeout -k 10 200 python bench.py --full --steps 10 --warmup 3 --no-extras ${BENCH_ARGS} 2>/dev/null | tail -1 | python -c "
import sys, json
d = json.loads(sys.stdin.read()); print('$f', d['value'], d['ratio'], d['roofline']['kernels_ms_per_step'])" || exit 1
    done
}
case "$mode" in
bench) bench ;;
l1)         # level-1 and 128 KiB bench lines of every variant
    for f in zstandard_amd/lib/var_*.so; do
      for args in "--level 1" "--level 1 --chunks 2048 --chunk-size 131072" "--chunks 2048 --chunk-size 131072"; do
        ZSMI_LIB_FILE=$PWD/$f timeout -k 10 200 python bench.py --full --steps 10 --warmup 3 --no-extras --no-cpu-baseline --decode-frames 0 $args 2>/dev/null | tail -1 | python -c "
import sys, json
d = json.loads(sys.stdin.read()); print('$f', '$args', d['value'], d['ratio'], d['roofline']['kernels_ms_per_step'])" || exit 1
      done
    done ;;
kernels)    # per-kernel compress times (no output check: timing-aid builds included); CLASSES="a b": on each of those data classes
    for f in zstandard_amd/lib/var_*.so; do
        if [ -z "$CLASSES" ]; then echo -n "$f "; ZSMI_LIB_FILE=$PWD/$f timeout -k 10 200 python tools/time_kernels.py 2>&1 | tail -1 || exit 1; fi
        for c in $CLASSES; do
            echo -n "$f " ; CLS=$c ZSMI_LIB_FILE=$PWD/$f timeout -k 10 200 python tools/time_kernels.py 2>/dev/null | tail -1 || exit 1
        done
    done ;;
decode)     # per-kernel decode times (no output check: timing-aid builds included)
    for f in zstandard_amd/lib/var_*.so; do
        ZSMI_LIB_FILE=$PWD/$f timeout -k 10 200 python tools/bench_decode.py --times-only --steps 3 "$@" 2>&1 | tail -1 || exit 1
    done ;;
check)      # encoder parity tests (HIP == oracle E) with var_NAME.so, then the bench line of every variant
    cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
    if [ -n "$1" ]; then
        ZSMI_LIB_FILE=$PWD/zstandard_amd/lib/var_$1.so timeout -k 10 600 python -m pytest tests/test_gpu_codec.py -m gpu -x -q -k "encode or mixed or zeros or units or joined or tiny or one_shot_large" > gpurun_out/check_$1.log 2>&1 || { tail -30 gpurun_out/check_$1.log; exit 1; }
        tail -3 gpurun_out/check_$1.log
    fi
    bench ;;
checkdec)   # decode parity tests with var_NAME.so, then the decode kernel times of every variant
    cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
    if [ -n "$1" ]; then
        ZSMI_LIB_FILE=$PWD/zstandard_amd/lib/var_$1.so timeout -k 10 600 python -m pytest tests/test_gpu_codec.py tests/test_gpu_fuzz.py -m gpu -x -q -k "(decode or fuzz or checksum or zeros or roundtrip) and not intended" > gpurun_out/checkdec_$1.log 2>&1 || { tail -30 gpurun_out/checkdec_$1.log; exit 1; }
        tail -2 gpurun_out/checkdec_$1.log
    fi
    for f in zstandard_amd/lib/var_*.so; do
        ZSMI_LIB_FILE=$PWD/$f timeout -k 5 300 python tools/bench_decode.py --times-only ${DEC_ARGS} 2>/dev/null | tail -1 || exit 1
    done ;;
*) echo "usage: tools/variants.sh bench | l1 | kernels | decode [flags] | check NAME | checkdec NAME" >&2; exit 2 ;;
esac
