// Which 1x1 convolutions of a block leave the tile engines for conv_ws.hip / conv_wl.hip, and on which grid each block asks.  Pure
// arithmetic (no HIP): the launchers of those two files check a launch with the same functions, and ace_sfno_create (which buffers
// exist), ace_sfno_set_weight (which fragments are packed) and plan_route (which kernel runs) ask one function per question - each
// with the grid the convolution runs on.  Compiled for the host by tests/emul/weight_prep_emul.cpp.
#pragma once

namespace ace {

// conv_ws.hip: weights resident in registers.  K: input channels (contraction), M: output channels; role 0 inner skip, 1 fc1, 2 fc2
// (-1: any); roles_on: Switches::conv_ws_roles.  HW enters through the 32-bit byte offsets of the output and of the statistics only
inline bool conv_ws_eligible(int K, int M, long HW, int role, int roles_on = 7) {
    if (role >= 0 && role < 3 && !(roles_on >> role & 1)) return false;
    if (role == -1 && roles_on == 0) return false;
    if (!(K == 128 || K == 256 || K == 384 || K == 512 || K == 768)) return false;
    if (role >= 0 && role <= 1 && K > 384) return false;
    return M % 128 == 0 && M >= 128 && M <= 2048 && (long)M * HW * 4 < 0x7fffff00L && ((HW + 31) / 32 + 8) * (long)M * 16 < 0x7fffff00L;
}
// conv_wl.hip: weights in LDS.  GELU + P-format output, no residual, no statistics (the first MLP convolution)
inline bool conv_wl_eligible(int K, int M, long HW) {
    if (K == 384) return M % 96 == 0 && M / 96 <= 32 && (long)M * HW * 2 < 0x7fffff00L;
    if (K == 512 || K == 256 || K == 128) return M % 64 == 0 && M / 64 <= 32 && (long)M * HW * 2 < 0x7fffff00L;   // two row tiles per workgroup (K = 512: 128 KiB of weights)
    return false;
}

// Role R of a K -> M convolution at HW pixels.  The last encoder convolution counts as an fc2 (static weights, fp32 residual,
// planes + statistics out); ws_roles / wl_on: Switches::conv_ws_roles / conv_wl
inline bool skip_on_conv_ws(int ws_roles, int K, int M, long HW) { return conv_ws_eligible(K, M, HW, 0, ws_roles); }
inline bool fc1_on_conv_ws(int ws_roles, int K, int M, long HW) { return conv_ws_eligible(K, M, HW, 1, ws_roles); }
inline bool fc2_on_conv_ws(int ws_roles, int K, int M, long HW) { return conv_ws_eligible(K, M, HW, 2, ws_roles); }
inline bool fc1_on_conv_wl(bool wl_on, int K, int M, long HW) { return wl_on && conv_wl_eligible(K, M, HW); }
// the inner skip of a noise-conditioned net (conv_ws.hip mode 6: no per-step weight fold, any K of that file): the "skip" bit of
// ACE_CONV_WS switches it
inline bool cln_skip_on_conv_ws(int ws_roles, int K, int M, long HW) {
    return (ws_roles & 1) && conv_ws_eligible(K, M, HW, -1, ws_roles);
}

// Pixels of the grid block i's skips, norm1 and MLP run on: what its filter's inverse transform produced - the data grid behind
// the last block, the inner (scale_factor) grid behind every other one (sfnonet.py:217-252)
inline long block_out_pixels(int i, int num_layers, long hw_data, long hw_inner) { return i == num_layers - 1 ? hw_data : hw_inner; }
// ... and a question asked "for any block of this net": q(pixels), over the grids the blocks run on
template <class Q>
inline bool any_block(int num_layers, long hw_data, long hw_inner, Q q) {
    for (int i = 0; i < num_layers; ++i)
        if (q(block_out_pixels(i, num_layers, hw_data, hw_inner))) return true;
    return false;
}

}  // namespace ace
