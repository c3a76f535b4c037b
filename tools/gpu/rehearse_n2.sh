#!/bin/bash
# the N = 2 code path of bench.py on a box with ONE GPU (both ranks on device 0, collectives over gloo): does every leg run?
O=${REHEARSE_OUT:-rehearse_out}
mkdir -p $O
SX_BENCH_REHEARSAL=gloo timeout -k 10 800 python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 \
  --master-port 29511 bench.py --gpus 2 --steps 5 --warmup 2 --full > $O/rehearse_n2.json 2> $O/rehearse_n2.err
rc=$?
tail -c 600 $O/rehearse_n2.err; echo
python - $O/rehearse_n2.json <<'PY'
import json
import sys
d = json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print({k: d[k] for k in ("metric", "value", "n_gpus", "ms_per_step", "scaling")})
print("sharded_pricing", d.get("sharded_pricing"))
print("sharded_resolve", d.get("sharded_resolve"))
PY
exit $rc
