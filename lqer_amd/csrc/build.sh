#!/bin/bash
# Build liblqer_hip.so for gfx950 (cross-compiles without a GPU).  Usage: build.sh [extra hipcc flags]
set -e
cd "$(dirname "$0")"
# (at most 16 jobs: nproc reports every CPU of a shared host, not the share a build may use)
J=$(nproc); [ "$J" -gt 16 ] && J=16
make -s -j"$J" EXTRA="$*"
echo "built $(realpath ../liblqer_hip.so)"
