#!/bin/bash
# Register / scratch footprint of every register instantiation (compile only), one line per kernel -- default blocks, 4-wave
# blocks, batch, reference width:  tools/resources.sh [extra flags]
cd "$(dirname "$0")/../monte_carlo_gp_amd/csrc"
one() {
  n=$1; shift
  /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -fno-fast-math -DMCGP_INST_N=$n "$@" -S --cuda-device-only \
    -o /tmp/res_$n.s reg_inst.hip -Rpass-analysis=kernel-resource-usage 2>&1 |
    awk -v n=$n '
      function flush() { if (k != "") printf "N=%2d %-6s vgpr=%3d scratch=%4d vgpr_spill=%3d sgpr_spill=%3d occupancy=%d\n", n, k, v, s, vs, ss, o }
      /Function Name/ { flush(); f = $(NF-1)
                        k = f ~ /race_kernel_reg_batch/ ? "batch" : f ~ /race_kernel_reg_wide/ ? "wide" : f ~ /race_kernel_regILi[0-9]+ELi4E/ ? "small" : "reg"
                        if (k == "small" && seen_reg == 0) k = "reg"      # (a field size whose default block is the 4-wave one)
                        if (k == "reg") seen_reg = 1 }
      / VGPRs:/{v=$(NF-1)} /ScratchSize/{s=$(NF-1)} /VGPRs Spill/{vs=$(NF-1)} /SGPRs Spill/{ss=$(NF-1)} /Occupancy/{o=$(NF-1)}
      END { flush() }'
}
export -f one
seq 1 32 | xargs -P 8 -I{} bash -c "one {} $*" | sort -t= -k2 -n -s
