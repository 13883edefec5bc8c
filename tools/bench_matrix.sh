#!/bin/bash
# bench.py --full over workloads, variants and batch sizes on one GPU; JSON lines into $OUT/matrix.jsonl (OUT defaults to bench_out)
R=$(cd "$(dirname "$0")/.." && pwd); cd $R; OUT=${OUT:-bench_out}; mkdir -p $OUT; : > $OUT/matrix.jsonl
# run [NAME=value ...] <bench.py arguments>: one row, headed by the switches and arguments it ran with
run() { local e=(); while [[ $1 == *=* ]]; do e+=("$1"); shift; done; echo "# ${e[*]:+${e[*]} }$*" >> $OUT/matrix.jsonl
        env "${e[@]}" timeout -k 10 300 python bench.py --full --no-cpu-baseline --no-extras "$@" 2>/dev/null | tail -1 >> $OUT/matrix.jsonl; }
timeout -k 10 400 python bench.py --full --steps 30 2>/dev/null | tail -1 > $OUT/matrix_default.json
run --steps 30
run --steps 30 --variant textured
run --steps 30 --variant sparse
run --steps 30 --variant natural
run --steps 30 --workload stereo640
run --steps 30 --workload stereo640_match
run --steps 30 --workload mono640_init
run --steps 30 --workload mono640_track
run --steps 30 --workload mono640_bow
run --steps 30 --workload mono640_refkf
run --steps 30 --workload mono640_bgr
run --steps 30 --workload hd720
run --steps 30 --workload hd1080
run --steps 30 --workload hd1080 --variant natural
run --steps 300 --batch 1
run --steps 300 --batch 2 --workload stereo640
run --steps 200 --batch 2 --workload stereo640_match
run --steps 200 --batch 2 --workload mono640_track
run --steps 200 --batch 2 --workload mono640_refkf
run --steps 200 --batch 2 --workload mono640_init
run --steps 200 --batch 8
run --steps 100 --batch 64
run --steps 60 --batch 128
run --steps 50 --batch 256
run --steps 15 --batch 1024
run --steps 10 --batch 2048
run ORBX_SPLIT=0 --steps 30
run ORBX_FUSE_SMALL=0 --steps 300 --batch 1
run ORBX_PATCH_BLUR=0 --steps 30 --workload hd1080
run ORBX_PATCH_BLUR=0 --steps 30 --workload hd720
run ORBX_SPLIT=3 --steps 30 --batch 256
run ORBX_PATCH_BLUR=0 --steps 30
run ORBX_BLUR_SPLIT=0 --steps 30
run ORBX_BLUR_SPLIT=4 --steps 30
run --steps 30 --handles 2
HOST_RATE_BATCHES=1,8,64,256,512 timeout -k 10 300 python tools/host_path_rate.py > $OUT/host_path.txt 2>&1
echo done
