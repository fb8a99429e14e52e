# the sampler probe (scripts/dev/sampler_sol.{hip,py}): the SQ counters of V2 / V5 - V9 in a
# counter-only pass, then the timed table with the counters merged in -> $OUT/sol_$TAG.json
#   hipcc -O3 -std=c++17 --offload-arch=gfx950 -shared -fPIC scripts/dev/sampler_sol.hip \
#         -o scripts/dev/libs/sol/libsampler_sol.so
#   TAG=r07a bash scripts/dev/gpu_sampler_sol.sh
set -o pipefail
cd "$(dirname "$0")/../.."; export TMPDIR=/tmp
TAG=${TAG:-r07a}; OUT=${OUT:-bench_out_sol}; mkdir -p $OUT
timeout -k 10 200 rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_INSTS_VALU -d $OUT/pmc_sol_$TAG -o run --output-format csv -- python3 scripts/dev/sampler_sol.py --variants 2,5,6,7,8,9 --reps 1 --no-real > $OUT/pmc_sol_$TAG.log 2>&1 || { tail -20 $OUT/pmc_sol_$TAG.log; exit 1; }
timeout -k 10 300 python scripts/dev/sampler_sol.py --merge-pmc $OUT/pmc_sol_$TAG > $OUT/sol_$TAG.json 2> $OUT/sol_$TAG.err || { tail -20 $OUT/sol_$TAG.err; exit 1; }
cat $OUT/sol_$TAG.json
echo done
