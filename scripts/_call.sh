O=${MZ_OUT_DIR:-bench_out}  # where the logs and result lines go
cd "$(dirname "$0")/.." && mkdir -p "$O"
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q -p no:cacheprovider --timeout 300 --timeout-method thread > $O/pytest_chain.log 2>&1; rc=$?; echo "pytest rc=$rc"; tail -25 $O/pytest_chain.log; [ $rc -gt 1 ] && exit $rc
for v in 0 1; do MZ_NO_CHAIN=$v timeout -k 10 300 python bench.py --full --no-cpu > $O/bench_chain$v.json 2>&1 || exit $?; python -c "
import json; d=json.loads(open('$O/bench_chain$v.json').read().strip().splitlines()[-1]); print('NO_CHAIN=$v', round(d['value']/1e6,2), 'M', d['roofline']['avg_launch_us'], 'us')"; done
