# Full GPU validation of the tree on one MI355X: every -m gpu test, smoke(), the bench line with everything beside the
# headline (--full), PMC traffic of the fused dwconv/gLN backward.
# usage (from the repo root): bash tools/gpu_validate.sh OUTDIR      (logs go to OUTDIR, default validate_out/)
out=${1:-validate_out}
mkdir -p "$out"; export HSA_ENABLE_IPC_MODE_LEGACY=0
timeout -k 10 900 python -u -m pytest tests -x -v -m gpu --timeout 300 --timeout-method thread > "$out/validate_tests.log" 2>&1; rc=$?
echo "tests rc=$rc"; grep -E "FAILED|ERROR|passed|failed" "$out/validate_tests.log" | tail -8
[ $rc -eq 0 ] || exit 1
timeout -k 10 300 python -u -c "import __graft_entry__ as g; g.smoke()" > "$out/validate_smoke.log" 2>&1; rc=$?; echo "smoke rc=$rc"; grep smoke "$out/validate_smoke.log"
[ $rc -eq 0 ] || exit 1
timeout -k 10 900 python -u bench.py --full > "$out/validate_bench.log" 2>&1; rc=$?; echo "bench rc=$rc"; grep '^{' "$out/validate_bench.log" | tail -1 | cut -c1-1500
[ $rc -eq 0 ] || exit 1
PHASES="cconv dwconv_gln dwconv_gln_bwd" bash tools/pmc_traffic.sh "$out/validate_pmc" "$out/validate_traffic.json" > "$out/validate_pmc.log" 2>&1; echo "pmc rc=$?"; tail -3 "$out/validate_pmc.log"
