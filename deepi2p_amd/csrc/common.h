// Shared host/device helpers for libdeepi2p_hip.so (gfx950 only; no portability layers).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/deepi2p_hip.h"

#define DI2P_WAVE 64

void di2p_set_error(const char* fmt, ...);

#define DI2P_CHECK_ARG(cond, msg)                                   \
    do {                                                            \
        if (!(cond)) {                                              \
            di2p_set_error("%s: %s", __func__, msg);                \
            return -1;                                              \
        }                                                           \
    } while (0)

#define DI2P_RETURN_LAUNCH()                                                        \
    do {                                                                            \
        hipError_t e_ = hipGetLastError();                                          \
        if (e_ != hipSuccess) {                                                     \
            di2p_set_error("%s: launch failed: %s", __func__, hipGetErrorString(e_)); \
            return (int)e_;                                                         \
        }                                                                           \
        return 0;                                                                   \
    } while (0)

static inline int di2p_cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }

// Tuning / test knobs.  Read ONCE from the environment (DI2P_<NAME>) when the library is first used and cached: no
// getenv() on the launch path.  Tests and tools flip them at run time through di2p_set_option().
// One list defines the knobs: X(ID, "name", "DI2P_<NAME>", default) gives the enumerator DI2P_OPT_<ID>, the name di2p_set_option() / di2p_get_option()
// take, the environment variable and the default (common.cpp builds its table from the same list).
#define DI2P_OPTIONS(X) \
    X(CONV_NOSPLIT, "conv_nosplit", "DI2P_CONV_NOSPLIT", 0)                       /* 1: never split K in the convolutions */ \
    X(CONV_DEPTH1, "conv_depth1", "DI2P_CONV_DEPTH1", 0)                          /* 1: depth-1 register prefetch in the vector convolution engine (default: depth 2; bit-identical) */ \
    X(PW_NOVEC, "pw_novec", "DI2P_PW_NOVEC", 0)                                   /* 1: scalar stager for the pointwise GEMMs */ \
    X(SOLVER_NOCULL, "solver_nocull", "DI2P_SOLVER_NOCULL", 0)                    /* 1: classify every cluster per point (bit-identical by construction) */ \
    X(SOLVER_NOPREFILTER, "solver_noprefilter", "DI2P_SOLVER_NOPREFILTER", 0)     /* 1: skip the fp32 pre-filter of the per-point classification (bit-identical by construction) */ \
    X(SOLVER_TIER_SWEEPS, "solver_tier_sweeps", "DI2P_SOLVER_TIER_SWEEPS", 0)     /* sweeps after which a hypothesis is handed to the wide (16-wave) tail kernel; 0 = never */ \
    X(WINO_COB, "wino_cob", "DI2P_WINO_COB", 0)                                   /* 32 / 64: force the output-channel block of the Winograd convolution (0: by grid size) */ \
    X(CONV_NOWINOGRAD, "conv_nowinograd", "DI2P_CONV_NOWINOGRAD", 0)              /* 1: the inference network runs 3x3 stride-1 convolutions on the direct implicit-GEMM kernel, not on Winograd (read by ops.conv_route; the training step does not read it) */ \
    X(WINO_KC, "wino_kc", "DI2P_WINO_KC", 0)                                      /* 8 / 4: input channels per K-step of the Winograd convolution (0: 4 up to 256 input channels, else 8) */ \
    X(CONV_NOSTEM, "conv_nostem", "DI2P_CONV_NOSTEM", 0)                          /* 1: the host layer runs the 7x7 stem on the generic implicit-GEMM kernel (read by networks.py) */ \
    X(WINO_REG, "wino_reg", "DI2P_WINO_REG", 0)                                   /* Winograd kernel: 0 automatic, 1 LDS-panel kernel, 2 register-resident (4 waves), 3 register-resident (2 waves) */ \
    X(SOLVER_NOCACHE, "solver_nocache", "DI2P_SOLVER_NOCACHE", 0)                 /* 1: no classification cache in the cluster walk (bit-identical by construction) */ \
    X(SOLVER_PREP_SINGLE, "solver_prep_single", "DI2P_SOLVER_PREP_SINGLE", 0)     /* 1: frame preparation as ONE workgroup per frame (the round-4 kernel; default: five multi-workgroup launches; same results) */ \
    X(SOLVER_PREP_BITONIC, "solver_prep_bitonic", "DI2P_SOLVER_PREP_BITONIC", 0)  /* 1: frame preparation always sorts with the bitonic network (default: counting sort + per-bucket ranking; same order) */ \
    X(PW_X3, "pw_x3", "DI2P_PW_X3", 1)                                            /* 1 (default): the host layer runs the GEMM-shaped pointwise layers (K >= 128, M % 128 == 0) on the bf16x3 kernel (read by ops.py) */ \
    X(PW_NOCHAIN, "pw_nochain", "DI2P_PW_NOCHAIN", 0)                             /* 1: the host layer runs the narrow PointNet chains as separate launches instead of di2p_point_chain (bit-identical; read by ops.py) */ \
    X(HEAD_REG, "head_reg", "DI2P_HEAD_REG", 0)                                   /* 1: di2p_point_head runs the wave-autonomous kernel (one persistent 8-wave workgroup per compute unit: faster alone, slower beside other streams' kernels) instead of the LDS-tile kernel (bit-identical) */ \
    X(CONV_S2SCALAR, "conv_s2scalar", "DI2P_CONV_S2SCALAR", 0)                    /* 1: stride-2 convolutions stage their operand with four dword loads per row (rounds 1-3) instead of aligned 8-float windows (bit-identical) */ \
    X(CONV_X3, "conv_x3", "DI2P_CONV_X3", 31)                                     /* bit mask of the 3x3 layers the host layer runs on di2p_conv3x3_x3 where it supports their shape (bf16 MFMA, exact three-way splits): bit s-1 = stride-1 layers of ResNet stage s, bit 4 = the stride-2 layers with their 1x1 downsample branch; 0: Winograd / direct fp32-MFMA kernels only (read by ops.conv_route, for inference and training alike) */ \
    X(CONV_X3_CFG, "conv_x3_cfg", "DI2P_CONV_X3_CFG", -1)                         /* >= 0: force tile configuration 0..3 of di2p_conv3x3_x3 where the call passes cfg = -1 (default -1: cheapest by a cost model) */ \
    X(HEAD_X3, "head_x3", "DI2P_HEAD_X3", 1)                                      /* 1 (default): the host layer runs the coarse per-point head on di2p_point_head_x3 (bf16 MFMA, exact three-way splits, wave-autonomous); 0: di2p_point_head (fp32 MFMA, LDS tile; bit-identical to the three separate launches) (read by networks.py) */ \
    X(HEAD_X3_TAB, "head_x3_tab", "DI2P_HEAD_X3_TAB", 1)                          /* 1 (default): di2p_point_head_x3 keeps the frame's two node tables in LDS, one workgroup of eight waves (two per SIMD, 256 registers) per compute unit; 2: the same with four waves (one per SIMD, 512 registers); 0: gathers the tables from memory (no LDS: shares its compute units) */ \
    X(STEM_X3, "stem_x3", "DI2P_STEM_X3", 1)                                      /* 1 (default): the host layer runs conv1 + bn1 + relu + max-pool of the image branch as ONE launch of di2p_stem_x3 (bf16 MFMA, exact three-way splits) where it supports the image size; 0: di2p_conv7x7s2_stem + di2p_maxpool3x3s2 (fp32 MFMA) (read by networks.py) */ \
    X(BN_UNFUSED, "bn_unfused", "DI2P_BN_UNFUSED", 0)                             /* 1: train-mode BatchNorm finalizes its statistics in a launch of its own (rounds 2-5; default: inside the elementwise pass, same results) */ \
    X(PW_X3_PLANES, "pw_x3_planes", "DI2P_PW_X3_PLANES", 1)                       /* 1 (default): consecutive bf16x3 pointwise layers hand their activations on as split bf16 planes (di2p_epilogue_t.planes_out -> di2p_pointwise_gemm_x3p) instead of fp32 (bit-identical; read by networks.py); 2: the same, and di2p_pointwise_gemm_x3p always runs its 128-row kernel (default: 256-row tiles with both operands in LDS when M % 256 == 0) */ \
    X(CONV_DGRAD_DENSE, "conv_dgrad_dense", "DI2P_CONV_DGRAD_DENSE", 0)           /* 1: di2p_conv2d_dgrad runs its dense kernel for stride 2 too (default: one parity class of input pixels per workgroup, 1/4 of the matrix work; same results) */ \
    X(RC_TILE64, "rc_tile64", "DI2P_RC_TILE64", 0)                                /* 1: the reduction GEMMs of the training step (weight gradients) always run 64 x 64 tiles (default: 128 x 128 for strided operand pairs with at least 128 rows and columns) */
enum Di2pOption {
#define DI2P_OPT_ENUM(ID, NAME, ENV, DEF) DI2P_OPT_##ID,
    DI2P_OPTIONS(DI2P_OPT_ENUM)
#undef DI2P_OPT_ENUM
    DI2P_OPT_COUNT
};
long long di2p_opt(int id);
int di2p_cu_count();      // compute units of the current device (cached per device)
// The opt-in a kernel needs for more than 64 KB of dynamic LDS (per device and cheap: made before every such launch, never cached).
// Refused: sets "<who>: <bytes> bytes of dynamic LDS refused: <hip error>", clears the sticky error and returns non-zero.
int di2p_allow_dynamic_lds(const void* kernel, size_t bytes, const char* who);
// (head_x3.hip) the bf16x3 split of Wt f32[K][M] (K % 16 == 0) in the A-fragment order of 32-row tiles, rows past M zero: the 3 KB entry of
// (row tile t, K-step s) at t * tile_stride + s * step_stride; launch only
void di2p_pack_a32(const float* Wt, int K, int M, int tiles, int tile_stride, int step_stride, void* Wp, void* stream);
