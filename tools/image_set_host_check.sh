#!/bin/bash
# The host half of the image-set edit under AddressSanitizer + UndefinedBehaviorSanitizer, outside Python: tools/image_set_host_check.cpp (its own main) with
# scene_image_set.cpp, scene_builder.cpp and the host sources they need, host code compiled -fsanitize=address,undefined.  CPU only: the program makes no HIP call.
#   tools/image_set_host_check.sh [output directory, default $TMPDIR or /tmp]
set -eu
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${1:-${TMPDIR:-/tmp}}
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
cd "$ROOT/cudatracerlib_amd/csrc"
SAN="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined"
"$HIPCC" --offload-arch=gfx950 -std=c++17 -O1 -g -ffp-contract=off -pthread $SAN -I. -x hip ../../tools/image_set_host_check.cpp \
    scene_image_set.cpp flat_mesh_set.cpp flat_meshes.cpp flat_nodes.cpp flat_rebuild.cpp flatten.cpp scene_builder.cpp scene_checks.cpp geometry_hash.cpp bvh_builder.cpp sbvh_builder.cpp scene_cache.cpp image_io.cpp jpeg_decode.cpp \
    -fsanitize=address,undefined -lz -ldl -o "$OUT/image_set_host_check"
"$OUT/image_set_host_check"
