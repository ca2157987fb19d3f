set -e
export TMPDIR=/tmp
O=${1:-prof_out/r06q}
mkdir -p $O/kt $O/kt1
timeout -k 10 500 rocprofv3 --kernel-trace --stats -d $O/kt -o run --output-format csv -- python3 bench.py --full > $O/bench_default_ktrace.log 2>&1
python3 tools/ktrace_summary.py $O/kt_tmp 2>/dev/null || true
timeout -k 10 400 rocprofv3 --kernel-trace --stats -d $O/kt1 -o run --output-format csv -- python3 bench.py --streams 1 --steps 1 --warmup 1 --no-parity --no-cpu-baseline --no-api-path > $O/kt1.log 2>&1
