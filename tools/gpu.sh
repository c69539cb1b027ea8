# One entry point for work on the MI355X host (run from the repo root).  Logs, traces and
# counter CSVs go to $ECG_OUT (default: out/ in the repo root; tools/pmc_summary.py reads the same).
#   bash tools/gpu.sh tests [pytest args]     -m gpu parity suite (+ smoke)
#   bash tools/gpu.sh bench [bench args]      one bench.py --full line -> $ECG_OUT/bench.log
#   bash tools/gpu.sh prof TAG                rocprofv3 kernel stats + FETCH/WRITE PMC passes
#   bash tools/gpu.sh sq TAG LOGN [COUNTERS]  one SQ counter pass over tools/msm_once.py
#   bash tools/gpu.sh round TAG               tests + smoke + bench + bn254 bench + prof
# Every GPU step runs under its own timeout and the steps are chained, so the
# first failure ends the call.
set -o pipefail
R=$PWD
OUT=${ECG_OUT:-$R/out}
mkdir -p $OUT
cmd=${1:-tests}; shift || true

tests() {
  timeout -k 10 1200 python3 -u -m pytest tests -x -v -m gpu --timeout 300 --timeout-method thread "$@" \
    > $OUT/pytest_gpu.log 2>&1; rc=$?; echo "pytest rc=$rc"; tail -3 $OUT/pytest_gpu.log
  [ $rc -eq 0 ] || return $rc
  timeout -k 10 300 python3 -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1; rc=$?
  echo "smoke rc=$rc"; tail -2 $OUT/smoke.log
  return $rc
}

bench() {
  timeout -k 10 600 python3 bench.py --full "$@" > $OUT/bench.log 2>&1; rc=$?
  echo "bench rc=$rc"; tail -1 $OUT/bench.log | cut -c1-1500
  return $rc
}

prof() {
  local TAG=$1
  ( cd /tmp && export TMPDIR=/tmp &&
    timeout -k 10 600 rocprofv3 --kernel-trace --stats -d $OUT/prof_$TAG -o run --output-format csv \
      -- python3 $R/bench.py --full --no-cpu-baseline --no-e2e --no-aux --no-table > $OUT/prof_${TAG}_bench.log 2>&1 &&
    echo trace-ok &&
    timeout -k 10 600 rocprofv3 --pmc FETCH_SIZE --kernel-trace -d $OUT/pmc_fetch_$TAG -o run \
      --output-format csv -- python3 $R/bench.py --full --no-cpu-baseline --no-e2e --no-aux --no-table --steps 1 --warmup 0 \
      > $OUT/pmc_fetch_${TAG}.log 2>&1 && echo fetch-ok &&
    timeout -k 10 600 rocprofv3 --pmc WRITE_SIZE --kernel-trace -d $OUT/pmc_write_$TAG -o run \
      --output-format csv -- python3 $R/bench.py --full --no-cpu-baseline --no-e2e --no-aux --no-table --steps 1 --warmup 0 \
      > $OUT/pmc_write_${TAG}.log 2>&1 && echo write-ok )
}

sq() {
  local TAG=$1 LOGN=$2
  local CTRS=${3:-"SQ_WAVES SQ_INSTS_VALU SQ_INSTS_VALU_INT32 SQ_INSTS_VALU_INT64 SQ_INSTS_SALU SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_INST_ANY"}
  ( cd /tmp && export TMPDIR=/tmp &&
    timeout -s KILL 300 rocprofv3 --pmc $CTRS --kernel-trace -d $OUT/sq_$TAG -o run --output-format csv \
      -- python3 $R/tools/msm_once.py $LOGN 1 > $OUT/sq_$TAG.log 2>&1 ) || { echo "sq $TAG failed"; return 1; }
  python3 $R/tools/sq_summary.py $OUT/sq_$TAG/run_counter_collection.csv | tee $OUT/sq_${TAG}_summary.txt
}

# one counter pass over any python target: pmc TAG "CTR ..." script.py args...
pmc() {
  local TAG=$1 CTRS=$2; shift 2
  ( cd /tmp && export TMPDIR=/tmp &&
    timeout -s KILL 300 rocprofv3 --pmc $CTRS --kernel-trace -d $OUT/pmc_$TAG -o run --output-format csv \
      -- python3 "$@" > $OUT/pmc_$TAG.log 2>&1 ) || { echo "pmc $TAG failed"; return 1; }
  echo "pmc $TAG ok"
}

# diagnostics: in-kernel clock (GRBM) + SQ instruction mix of the MSM accumulate
# (both curves) and of the NTT pass
diag() {
  local TAG=$1 SQ1="SQ_WAVES SQ_INSTS_VALU SQ_INSTS_VALU_INT64 SQ_INSTS_VALU_INT32 SQ_INSTS_SALU SQ_INSTS_LDS SQ_WAVE_CYCLES SQ_WAIT_INST_ANY"
  local SQ2="SQ_WAVES SQ_BUSY_CYCLES SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS SQ_WAIT_INST_LDS SQ_LDS_BANK_CONFLICT SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR"
  pmc ${TAG}_clk_bls "GRBM_GUI_ACTIVE GRBM_COUNT" $R/tools/msm_once.py 26 16 1 bls12_381 &&
  pmc ${TAG}_clk_bn "GRBM_GUI_ACTIVE GRBM_COUNT" $R/tools/msm_once.py 26 20 1 bn254 &&
  pmc ${TAG}_sq_bls "$SQ1" $R/tools/msm_once.py 24 1 1 bls12_381 &&
  pmc ${TAG}_sq_bn "$SQ1" $R/tools/msm_once.py 24 1 1 bn254 &&
  pmc ${TAG}_clk_ntt "GRBM_GUI_ACTIVE GRBM_COUNT" $R/tools/ntt_once.py 24 1000 &&
  pmc ${TAG}_sq_ntt "$SQ1" $R/tools/ntt_once.py 24 3 &&
  pmc ${TAG}_sq2_ntt "$SQ2" $R/tools/ntt_once.py 24 3
}

# BN254 counter passes (bench line's BN254 roofline.traffic): accumulate at 2^26, NTT at 2^24
bnpmc() {
  local TAG=$1
  pmc ${TAG}_bn_acc_fetch "FETCH_SIZE" $R/tools/msm_once.py 26 1 1 bn254 &&
  pmc ${TAG}_bn_acc_write "WRITE_SIZE" $R/tools/msm_once.py 26 1 1 bn254 &&
  pmc ${TAG}_bn_ntt_fetch "FETCH_SIZE" $R/tools/ntt_once.py 24 3 bn254_fr &&
  pmc ${TAG}_bn_ntt_write "WRITE_SIZE" $R/tools/ntt_once.py 24 3 bn254_fr
}

case $cmd in
  tests) tests "$@" ;;
  bench) bench "$@" ;;
  prof) prof "$@" ;;
  sq) sq "$@" ;;
  diag) diag "$@" ;;
  bnpmc) bnpmc "$@" ;;
  round)
    TAG=$1
    tests && bench && {
      timeout -k 10 600 python3 bench.py --full --curve bn254 --no-e2e > $OUT/bench_bn254.log 2>&1; rc=$?
      echo "bn254 bench rc=$rc"; [ $rc -eq 0 ]; } && prof $TAG ;;
  *) echo "unknown subcommand $cmd"; exit 2 ;;
esac
