#!/usr/bin/env bash
# Times pre-built library variants (tools/build_variant.sh) inside ONE gpurun call, interleaved, first variant repeated last.
#   /usr/local/graft/bin/gpurun --timeout 900 -- 'CHECK="c1_raster or mirror" bash tools/ab_libs.sh base sym symtab'
# A variant whose run fails or exceeds BENCH_TIMEOUT seconds ends the whole comparison: nothing more is started on the GPU after it.
set -o pipefail
cd "${GRAFT_REPO_ROOT:-.}"; R=$(pwd)
for v in "$@" "$1"; do
  export DNSPLAT_LIB=$R/gpurun_ab/lib_$v.so
  if [ -n "${CHECK:-}" ]; then timeout 900 python -m pytest tests -m gpu -x -q -k "$CHECK" 2>&1 | tail -2 || exit 1; fi
  for rep in 1 2; do
    timeout -k 10 ${BENCH_TIMEOUT:-300} python bench.py --full --no-cpu-baseline --steps ${STEPS:-30} --warmup 5 ${BENCH_ARGS:-} 2>/dev/null | tail -1 | python -c "
import json,sys
d=json.loads(sys.stdin.read())
st=d['stages']
print('$v |', d['value'], 'fps', d['ms_per_step'], 'ms | ' + ' '.join('%s %.4f' % (k.replace('dnsplat_',''), v['ms']) for k, v in st.items())
      + ' | careful loops %s' % d['config'].get('alpha_clamp_twin_active'))" || exit 1
  done
done
