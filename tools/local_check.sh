# LOCAL backward parity subset + Reddit bench (LOCAL and AUTO); development helper
mkdir -p bench_out
timeout -k 10 600 python -m pytest tests -q -m gpu -k "local or edge_cases or golden or backward" > bench_out/lc_tests.log 2>&1; rc=$?; tail -3 bench_out/lc_tests.log; [ $rc -eq 0 ] || exit $rc
timeout -k 10 300 python bench.py --full --bwd-algo local --no-cpu-baseline --steps 10 > bench_out/lc_local.json 2> bench_out/lc_local.err || exit $?
python -c "import json;d=json.load(open('bench_out/lc_local.json'));print('local', d['ms_per_step'], d.get('bwd_ms'), d.get('fwd_ms'))"
