#!/bin/bash
# Round-4 profiling session on the GPU box (bash tools/profile_r4.sh through gpurun, from the repo root); raw output under
# gpurun_out/prof_r4, summaries are copied into profiles/r4_final by `python tools/collect_r3.py gpurun_out/prof_r4 profiles/r4_final`.
# Every rocprofv3 runs the program directly after `--` (no env / shell wrapper), counters in their own passes with --kernel-trace only.
set -eu
: "${GRAFT_REPO_ROOT:?run through gpurun (GRAFT_REPO_ROOT is the repo copy on the GPU box)}"
R="$GRAFT_REPO_ROOT"
O="$R/gpurun_out/prof_r4"
rm -rf "$O" && mkdir -p "$O"
cd /tmp && export TMPDIR=/tmp
export MANNER_HIP_STREAMS=1        # single stream: launch durations are not inflated by the second stream
B="python3 $R/bench.py --full --warmup 1 --no-cpu --no-kernel-profile --no-table --no-collate --no-small-ops --no-train --no-dropin"
timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d "$O/stats" -- $B --steps 3 > "$O/stats.log" 2>&1; echo "stats done"
timeout -k 10 240 rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d "$O/fetch" -- $B --steps 1 > "$O/fetch.log" 2>&1; echo "fetch done"
timeout -k 10 240 rocprofv3 --kernel-trace --pmc WRITE_SIZE --output-format csv -d "$O/write" -- $B --steps 1 > "$O/write.log" 2>&1; echo "write done"
timeout -k 10 240 rocprofv3 --kernel-trace --pmc SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_VALU_MFMA_BUSY_CYCLES SQ_INSTS_LDS SQ_LDS_BANK_CONFLICT --output-format csv -d "$O/sq" -- $B --steps 1 > "$O/sq.log" 2>&1; echo "sq done"
unset MANNER_HIP_STREAMS
# the tail kernels at evaluation scale: scorer on the 495 MB table, one-pass and strict pooler, dot, z-score, to_dense, phase C in one launch vs separate
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$O/tail_stats" -- python3 "$R/tools/tail_probe.py" > "$O/tail_probe.json" 2> "$O/tail_stats.log"; echo "tail stats done"
timeout -k 10 300 rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d "$O/tail_fetch" -- python3 "$R/tools/tail_probe.py" > /dev/null 2> "$O/tail_fetch.log"; echo "tail fetch done"
timeout -k 10 300 rocprofv3 --kernel-trace --pmc WRITE_SIZE --output-format csv -d "$O/tail_write" -- python3 "$R/tools/tail_probe.py" > /dev/null 2> "$O/tail_write.log"; echo "tail write done"
# the training-step leg alone, ONE stream
export MANNER_HIP_STREAMS=1
timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d "$O/train" -- python3 "$R/bench.py" --full --steps 1 --warmup 0 --no-cpu --no-table --no-scale-parity --no-small-ops --no-collate --no-kernel-profile --no-dropin > "$O/train.log" 2>&1; echo "train done"
find "$O" -name "*kernel_trace.csv" -size +4M -delete
du -sh "$O"
