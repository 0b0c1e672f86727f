#!/bin/bash
# Compact register / scratch report of one translation unit: tools/kernel_regs.sh spx_bwd_npb6 [filter-regex]
# (hipcc -Rpass-analysis=kernel-resource-usage; one line per kernel instance: name, VGPRs, SGPRs, scratch bytes per lane, static LDS
# bytes, occupancy in waves per SIMD; checksums of the code itself: tools/device_code.py)
cd "$(dirname "$0")/../scaleprotoseg_amd/csrc" || exit 1
hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off $SPX_EXTRA_HIPCC_FLAGS -Rpass-analysis=kernel-resource-usage -c "$1.hip" -o /tmp/$1.regs.o 2> /tmp/$1.rpass
awk '/Function Name|Name: /{n=$0; sub(/.*Name: /,"",n); sub(/ \[.*/,"",n)} / VGPRs: /{v=$0; sub(/.* VGPRs: /,"",v); sub(/ .*/,"",v)} /TotalSGPRs: /{g=$0; sub(/.*: /,"",g); sub(/ .*/,"",g)} /ScratchSize/{s=$0; sub(/.*: /,"",s); sub(/ .*/,"",s)} /Occupancy/{o=$0; sub(/.*: /,"",o); sub(/ .*/,"",o)} /LDS Size/{l=$0; sub(/.*: /,"",l); sub(/ .*/,"",l); print n, "vgpr=" v, "sgpr=" g, "scratch=" s, "lds=" l, "occ=" o}' /tmp/$1.rpass | grep -E "${2:-.}"
