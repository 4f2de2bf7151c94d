#!/bin/bash
# GPU box: per-layer HBM-side traffic of the conv launches (two --pmc passes + the launch order of the instrumented frame)
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-out}
TAG=${1:-f16x3}
cd /tmp && export TMPDIR=/tmp
mkdir -p $R/$OUT; rm -rf $R/$OUT/pmc_fetch $R/$OUT/pmc_write
rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $R/$OUT/pmc_fetch -o pmc -- python $R/bench.py --full --steps 1 --warmup 1 --single-stream --no-cpu-baseline --no-extras --conv-table $R/$OUT/conv_table_pmc.txt > /dev/null 2> $R/$OUT/pmc_fetch.err
rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $R/$OUT/pmc_write -o pmc -- python $R/bench.py --full --steps 1 --warmup 1 --single-stream --no-cpu-baseline --no-extras > /dev/null 2> $R/$OUT/pmc_write.err
cd $R
python tools/pmc_traffic.py $OUT/pmc_fetch $OUT/pmc_write 5 > $OUT/pmc_traffic_$TAG.json 2> $OUT/pmc_traffic.err
python tools/pmc_per_layer.py $OUT/conv_table_pmc.txt.ordered.json $OUT/pmc_fetch $OUT/pmc_write > $OUT/traffic_per_layer_$TAG.txt 2>> $OUT/pmc_traffic.err
find $OUT/pmc_fetch $OUT/pmc_write -name "*kernel_trace.csv" -delete
find $OUT/pmc_fetch $OUT/pmc_write -name "*counter_collection.csv" -size +20M -delete
