# Round-end style confirmation on one MI355X: GPU tests, smoke, the full bench, rocprofv3 kernel statistics.
# Usage: bash tools/gpu_confirm.sh [TAG]   (logs: $VBC_LOG_DIR/TAG_*, default logs/)
# Test failures (pytest rc 1) are reported and the rest still runs; any other failure ends the script.
tag=${1:-confirm}
out=${VBC_LOG_DIR:-logs}
mkdir -p "$out"
export TMPDIR=/tmp
timeout -k 10 600 python -u -m pytest tests -m gpu -q --timeout 120 --timeout-method thread \
    -p no:cacheprovider > "$out/${tag}_gpu_tests.log" 2>&1
rc=$?
grep -E "^FAILED|passed|failed" "$out/${tag}_gpu_tests.log" | tail -20
case $rc in 0|1) ;; *) exit $rc ;; esac
timeout -k 10 180 python -u -c "import __graft_entry__ as g; g.smoke()" > "$out/${tag}_smoke.log" 2>&1 || exit $?
timeout -k 10 420 python -u bench.py --full > "$out/${tag}_bench.log" 2>&1 || exit $?
tail -c 1500 "$out/${tag}_bench.log"
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$out/${tag}_prof" -o run -- \
    python -u bench.py --full --no-cpu-baseline > "$out/${tag}_prof_bench.log" 2>&1 || exit $?
exit $rc
