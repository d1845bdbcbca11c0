#!/bin/bash
# bench.py --full (for its pcie_inclusive extra) at OW_PIPE = 1, 2, 4; the lines and logs go to the directory given as $1
O=${1:?usage: tools/pcie_probe.sh OUTDIR}; mkdir -p "$O"
for np in 1 2 4; do
  OW_PIPE=$np python bench.py --steps 20 --warmup 5 --full --no-cpu-baseline > "$O/pcie_$np.json" 2> "$O/pcie_$np.err"
  python - <<PY
import json
d=json.load(open("$O/pcie_$np.json"))
print("OW_PIPE=$np", "%.3e" % d["value"], "%.2f ms/step" % d["ms_per_step"], "pcie_inclusive %.3e %.2f ms" % (d["pcie_inclusive"]["value"], d["pcie_inclusive"]["ms_per_step"]))
PY
done
