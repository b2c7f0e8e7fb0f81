#!/bin/bash
# How the files of this directory were measured: from the repository root, after `make -C native`,
# on one MI355X with nothing else running on it. Each GPU step under its own time limit.
set -o pipefail
OUT=profiles/memprobe
timeout -k 10 240 python -m amdvgpu memprobe > $OUT/memprobe_cli.txt \
 && timeout -k 10 240 python -m amdvgpu run --cu 25 --memory 16g -- python -m amdvgpu memprobe > $OUT/memprobe_cli_cu25.txt \
 && timeout -k 10 800 python benchmarks/mem_interference.py --repeats 3 --limit 700 \
      --json-out $OUT/mem_interference.json --md-out $OUT/mem_interference.md
