#!/bin/bash
python "$(dirname "$0")/../bench.py" --steps 5 --warmup 2 --full --no-cpu-baseline --skip-extras 2>&1 | grep "^BENCH_DETAIL " | cut -d' ' -f2- | python -c "import json,sys; d=json.loads(sys.stdin.read()); print('sampler_ms', d['sampler_ms_per_batch'], 'value', d['value'])"
