#!/bin/bash
# One GPU-box session: parity tests, smoke, bench.  Stops at the first step
# that ends abnormally (fault/abort/timeout) — an assertion failure (rc 1)
# does not stop it.  Logs go to $OUT_DIR (default: bench_out).
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
out=${OUT_DIR:-bench_out}
mkdir -p $out
ok() { local rc=$1; [ "$rc" -eq 0 ] || [ "$rc" -eq 1 ]; }
timeout -k 10 400 python -u -m pytest tests/test_gpu.py -v --timeout 150 --timeout-method thread ${PYTEST_ARGS:-} > $out/gpu_tests.log 2>&1
rc=$?; echo "pytest rc=$rc"; tail -25 $out/gpu_tests.log
ok $rc || exit $rc
timeout -k 10 120 python -u -c "import __graft_entry__ as g; g.smoke()" > $out/smoke.log 2>&1
rc=$?; echo "smoke rc=$rc"; tail -5 $out/smoke.log
ok $rc || exit $rc
timeout -k 10 300 python -u bench.py --full ${BENCH_ARGS:-} > $out/bench.log 2>&1
rc=$?; echo "bench rc=$rc"; tail -5 $out/bench.log
exit $rc
