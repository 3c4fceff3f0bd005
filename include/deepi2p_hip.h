/*
 * deepi2p_hip.h -- C ABI of libdeepi2p_hip.so: the MI355X (gfx950) implementation of the
 * DeepI2P registration hot path.  Plain pointers and sizes only; every pointer is a DEVICE
 * pointer (HBM) unless the name ends in _host; `stream` is a hipStream_t passed as void*
 * (NULL = the null stream).  No function allocates, frees or synchronises: all are safe to
 * capture into a hipGraph.  Return value: 0 on success, otherwise a hipError_t / negative
 * argument-check code; di2p_last_error() returns a static description.
 *
 * Each entry point names the reference interface (path:line under lijx10/DeepI2P) it replaces.
 * INTEGRATION.md shows the binding a maintainer of the reference would add.
 *
 * Tensor layouts are the reference's own: point features f32 [B,C,N] (N contiguous), images
 * f32 NCHW, indices i32.
 */
#ifndef DEEPI2P_HIP_H
#define DEEPI2P_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

const char* di2p_last_error(void);
int di2p_version(void);
/* Tuning / test knobs, cached in the library (initialised once from the environment variable DI2P_<NAME>; what each one does is written
 * on its entry of the one table that defines them, DI2P_OPTIONS in deepi2p_amd/csrc/common.h):
 *   "conv_nosplit", "conv_depth1", "pw_novec", "solver_nocull", "solver_noprefilter", "solver_tier_sweeps", "wino_cob", "conv_nowinograd",
 *   "wino_kc", "conv_nostem", "wino_reg", "solver_nocache", "solver_prep_single", "solver_prep_bitonic", "pw_x3", "pw_nochain", "head_reg",
 *   "conv_s2scalar", "conv_x3", "conv_x3_cfg", "head_x3", "head_x3_tab", "stem_x3", "bn_unfused", "pw_x3_planes", "conv_dgrad_dense",
 *   "rc_tile64".
 * set: 0, or -1 for an unknown name; get: the value, or -1 for an unknown name. */
int di2p_set_option(const char* name, long long value);
long long di2p_get_option(const char* name);

/* ---------------------------------------------------------------------------------------------
 * index_max  -- replaces models/index_max_ext: index_max.cpp:141-148 (forward_cuda_shared_mem),
 * :132-139 (forward_cuda); kernels index_max_cuda.cu:10-26, :30-62.
 *   data f32[B,C,N], index i32[B,N] with values in [0,K)  ->  max_idx i32[B,C,K]
 *   max_idx[b,c,k] = first n with index[b,n]==k attaining max(data[b,c,n]) ; floor -1000 ;
 *   empty cluster (or nothing > -1000) -> 0.
 * di2p_index_max_values additionally writes the maxima themselves with empty clusters zeroed,
 * i.e. data.gather(2,max_idx) * mask_row_max of models/networks_pc.py:91-92,103-104 (max_idx may
 * be NULL there; mask f32[B,K] = mask_row_max from di2p_cluster_stats, or NULL = "a node is
 * non-empty iff something beat the floor").  `workspace` must hold B*C*K uint64 (scratch, contents undefined after). */
int di2p_index_max_forward(const float* data, const int32_t* index, int32_t* max_idx,
                           int B, int C, int N, int K, void* workspace, void* stream);
int di2p_index_max_values(const float* data, const int32_t* index, const float* mask, float* max_val,
                          int32_t* max_idx, int B, int C, int N, int K, void* workspace, void* stream);

/* ---------------------------------------------------------------------------------------------
 * ball_query -- replaces models/ball_query_ext: ball_query.cpp:33-39 (forward_cuda_shared_mem),
 * kernel ball_query_cuda.cu:11-50.  node_to_point_dist f32[B,M,N] -> i32[B,M,K]: first K point
 * ids (ascending n) with dist <= radius, cyclically padded; all zero when none. */
int di2p_ball_query_forward(const float* node_to_point_dist, int32_t* out_idx, float radius, int K,
                            int B, int M, int N, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Point <-> node kernels of PCEncoder / KeypointDetector.
 *
 * di2p_knn_nodes: the dense-distance + torch.topk(k smallest, sorted) idiom of
 *   models/networks_pc.py:61-65, models/networks_united.py:158-161,176-178,
 *   models/layers_pc.py:798-799.   query f32[B,3,Nq], nodes f32[B,3,M] ->
 *   idx i32[B,Nq,k].  The k neighbours are SELECTED by (squared distance, node id) and WRITTEN in
 *   ascending (distance, node id), distance = the rounded fp32 root of the fp32 squared distance
 *   (dx*dx + dy*dy) + dz*dz: exact ties go to the lower node id, and two nodes whose squared
 *   distances differ but whose roots round to the same float are told apart only at the k-th
 *   place.  One rule for every B, Nq, M.  weights (may be NULL) f32[B,Nq,k]
 *   = 1 - d_k/sum_j d_j, the interpolation weights of networks_united.py:97-98.
 *   k <= 16, k <= M <= 4096.
 * di2p_cluster_stats: networks_pc.py:66-76.  pc f32[B,3,N], knn idx (nearest = idx[b,n,0], row
 *   stride idx_stride) -> cluster_mean f32[B,3,M] = sum/(count+1e-5), mask f32[B,M] (1 if the
 *   node owns >=1 point), min_idx i32[B,N] (compact copy of the nearest id).
 * di2p_build_point_input: networks_pc.py:79-85.  -> pc_centers f32[B,3,N],
 *   augmented f32[B,7,N] = cat(pc - centers, intensity, sn).
 * di2p_interpolate: networks_united.py:90-103 (upsample_by_interpolation given idx+weights):
 *   feats f32[B,C,M] -> out f32[B,C,Nq] = sum_k w[b,n,k] * feats[b,c,idx[b,n,k]].
 * di2p_gather_neighbors: layers_pc.py:800-807 coordinates part: out f32[B,3,Mq*K] =
 *   database[:, idx] - query.
 * di2p_argmax_channels: multimodal_classifier.py:115-116.  scores f32[B,C,N] -> i32[B,N], first
 *   maximum wins. */
int di2p_knn_nodes(const float* query, const float* nodes, int32_t* idx, float* weights,
                   int B, int Nq, int M, int k, void* stream);
int di2p_cluster_stats(const float* pc, const int32_t* knn_idx, int idx_stride, float* cluster_mean,
                       float* mask, int32_t* min_idx, int B, int N, int M, void* stream);
int di2p_build_point_input(const float* pc, const float* intensity, const float* sn,
                           const float* cluster_mean, const int32_t* min_idx, float* pc_centers,
                           float* augmented, int B, int N, int M, void* stream);
int di2p_interpolate(const float* feats, const int32_t* idx, const float* weights, float* out,
                     int B, int C, int M, int Nq, int k, void* stream);
int di2p_gather_neighbors(const float* database, const float* query, const int32_t* idx, float* out,
                          int B, int Md, int Mq, int K, void* stream);
int di2p_argmax_channels(const float* scores, int32_t* out, int B, int C, int N, long long batch_stride /* elements; 0 = C*N */, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Pointwise contraction = EquivariantLayer / MyConv2d(1x1) (+BN eval +ReLU) of
 * models/layers_pc.py:259-342, :110-190, with the torch.cat / expand / gather feeding it
 * (networks_pc.py:98, layers_pc.py:808-813, networks_united.py:139-197) folded into the operand
 * loader.  fp32 in, fp32 MFMA (v_mfma_f32_32x32x2_f32) accumulate, fp32 out.
 *
 *   Y[b,m,n'] = epi( sum_k Wt[k,m] * X[b,k,n] )        n' = n, or n / group_max when group_max > 1
 *   epi(a)    = relu?( scale[m]*(a + batch_bias[b,m] + sum_t sum_j gw_t[b,n,j]*G_t[b,m,gidx_t[b,n,j]]) + shift[m] )
 *   (scale/shift = folded BatchNorm(eval) + conv bias; the batch_bias and gathered terms are part of
 *   the pre-activation, i.e. they stand for input channels that were never materialised)
 *
 * X is the virtual concatenation along k of up to DI2P_MAX_SRC sources.  Wt is the layer weight
 * transposed to [K,M] (packed once at load time).  group_max > 1 takes the max over each run of
 * `group_max` consecutive columns (torch.max(dim=3) of layers_pc.py:811,816). */
#define DI2P_MAX_SRC 3
#define DI2P_MAX_GK 16      /* = the k limit of di2p_knn_nodes */
enum { DI2P_SRC_DENSE = 0,   /* X[b,c,n]      = ptr[b*batch_stride + c*row_stride + n]            */
       DI2P_SRC_GATHER = 1,  /* X[b,c,n]      = ptr[b*batch_stride + c*row_stride + gidx[b,n]]    */
       DI2P_SRC_GROUP = 2    /* X[b,c,n]      = ptr[b*batch_stride + c*row_stride + n / group]    */ };
typedef struct {
    const float* ptr;
    const int32_t* gidx;     /* GATHER: i32[B, N] (batch stride = N) */
    long long batch_stride;  /* elements */
    int row_stride;          /* elements */
    int channels;
    int mode;
    int group;               /* GROUP mode divisor */
    int pad_;
} di2p_src_t;

typedef struct {
    const float* scale;        /* [M] or NULL (=1) */
    const float* shift;        /* [M] or NULL (=0) */
    const float* batch_bias;   /* [B,M] or NULL    */
    int relu;
    int group_max;             /* 1 = none */
    /* optional gathered add (per_point_pn layer 0 with W*interp == interp(W*nodes)):            */
    const float* g_table[2];   /* each f32[B,g_nodes,M] (node-major, M % 4 == 0; what transpose_out writes) or NULL */
    const int32_t* g_idx[2];   /* i32[B,N,g_k[t]] */
    const float* g_w[2];       /* f32[B,N,g_k[t]], or NULL for unit weights (plain gather) */
    int g_nodes[2];
    int g_k[2];                /* neighbours per column of each table, 1..DI2P_MAX_GK (the two tables may differ:
                                  opt.k_interp_point_a / k_interp_point_b, networks_united.py:158-165,188-191) */
    int transpose_out;         /* 1: Y is written f32[B,N,M] (needs M % 4 == 0, group_max == 1) */
    float* group_max_out;      /* with group_max > 1: NULL -> Y holds the maxima [B,M,N/group_max]; else Y is written in full
                                  [B,M,N] and the maxima go here (layers_pc.py:809-813 needs both) */
    void* planes_out;          /* (ABI 6; the bf16x3 entry points only, NULL elsewhere) not NULL: the full-size output [B,M,N] is written
                                  HERE, already split for the layer that contracts over it, instead of to Y as fp32:
                                  u16[B][3][M/4][N][4] = three bf16 planes (x = x1 + x2 + x3, exact), four consecutive rows of one
                                  column per 8 bytes; di2p_bf16x3_planes_bytes(B, M, N) bytes, 16-byte aligned, M % 4 == 0, no
                                  transpose_out.  Y then only receives the group maxima (group_max > 1 and group_max_out == NULL) and
                                  may be NULL otherwise. */
} di2p_epilogue_t;
/* Alignment: every g_table must be 16-byte aligned (all kernels read gathered rows 16 bytes at a time); the bf16x3 entry points
 * (di2p_pointwise_gemm_x3 / _x3p) also need scale, shift and batch_bias 16-byte aligned, with M % 4 == 0 for the batch_bias rows. */

int di2p_pointwise_gemm(const di2p_src_t* srcs_host, int n_src, const float* Wt, float* Y,
                        int B, int M, int K, int N, const di2p_epilogue_t* epi_host, void* stream);
/* The same contraction on the bf16 matrix instructions with an EXACT three-way split of both fp32 operands (x = x1 + x2 + x3, three truncated
 * bf16 terms; six bf16 products per fp32 product, fp32 accumulation): as accurate against an fp64 contraction as the fp32-MFMA kernel, 2.67x
 * its matrix-pipe rate.  For the GEMM-shaped layers (Conv1d / Conv2d(1x1) of models/layers_pc.py:259-408,779-818 with K >= 128 input
 * channels); the weights are split once:  Wp = di2p_bf16x3_pack(Wt [K][M])  (di2p_bf16x3_packed_bytes(K, M) bytes, 16-byte aligned).
 * Same sources, epilogues and output layouts as di2p_pointwise_gemm; needs M % 4 == 0 and N % 4 == 0. */
long long di2p_bf16x3_packed_bytes(int K, int M);
int di2p_bf16x3_pack(const float* Wt, int K, int M, void* Wp, void* stream);
/* (ABI 6, training) the split tap-major matrix of a 3x3 filter bank W f32[Cout][Cin][3][3] for di2p_conv3x3_x3, straight from W:
 * dgrad == 0: of the forward filter ([9 Cin, Cout]); dgrad == 1: of the filter that computes the layer's INPUT gradient as a convolution of
 * dY ([9 Cout, Cin]: taps flipped, channel roles swapped; models/resnet.py:56-72 under autograd).  Same bytes as di2p_bf16x3_pack of that matrix. */
int di2p_bf16x3_pack_conv3x3(const float* W, int Cout, int Cin, int dgrad, void* Wp, void* stream);
int di2p_pointwise_gemm_x3(const di2p_src_t* srcs_host, int n_src, const void* Wp, float* Y,
                           int B, int M, int K, int N, const di2p_epilogue_t* epi_host, void* stream);
/* A chain of such layers (GeneralKNNFusionModule's layers_before.1 -> layers_after.0 -> layers_after.1, models/layers_pc.py:779-818) hands
 * its activations on ALREADY SPLIT: the producer's epilogue writes planes_out (6 bytes per value instead of 4), the consumer stages them into
 * LDS without arithmetic -- the split leaves the K loop and is done once per value instead of once per 128-row block of every consumer.
 * `planes` = a planes_out of a layer with K rows and the same N; K % 32 == 0, N % 128 == 0.  Same epilogues (planes_out included) and, on the
 * same values, the same bits as di2p_pointwise_gemm_x3 with that layer's fp32 output as its one dense source. */
long long di2p_bf16x3_planes_bytes(int B, int C, int N);
int di2p_pointwise_gemm_x3p(const void* planes, const void* Wp, float* Y,
                            int B, int M, int K, int N, const di2p_epilogue_t* epi_host, void* stream);

/* Y[b,m] = sum_k Wt[k0+k, m] * v[b,k]  (the broadcast part of a concatenated input, folded into
 * batch_bias: networks_united.py:139-155,170-187 expand()s).  v f32[B,Kv]. */
/* Fused per-point head (per_point_pn, networks_united.py:57-74,194-197, coarse variant): three pointwise layers in
 * one launch, out = L2(L1(L0(concat(srcs)))) with
 *   L0: K0 dense channels -> M = 128, epilogue epi0 (scale/shift/relu, batch_bias, gathered node tables),
 *   L1: 128 -> 128 (W1t f32[128,128] k-major, scale1/shift1, relu1),   L2: 128 -> P <= 4 (W2t f32[128,P], scale2/shift2 or NULL).
 * out f32[B,P,N].  Bit-identical to three di2p_pointwise_gemm calls; the hidden activations stay in LDS. */
int di2p_point_head(const di2p_src_t* srcs_host, int n_src, const float* W0t, int K0, const di2p_epilogue_t* epi0_host,
                    const float* W1t, const float* scale1, const float* shift1, int relu1,
                    const float* W2t, const float* scale2, const float* shift2, int relu2,
                    float* out, int B, int M, int P, int N, void* stream);

/* Fused narrow PointNet chain (first_pointnet / second_pointnet of PCEncoder, networks_pc.py:36-43,60-75): two or three pointwise
 * layers of one width M (32 or 64) in one launch, Y = L2(L1(L0(src))) or L1(L0(src)) when W2t == NULL, with
 *   L0: ONE dense source of K0 <= M channels -> M, epilogue epi0 (scale/shift/relu, batch_bias, gathered node tables);
 *   L1, L2: M -> M (W1t / W2t f32[M,M] k-major, scale/shift may be NULL).  Y f32[B,M,N].
 * Bit-identical to the separate di2p_pointwise_gemm calls (up to the sign of zero); the hidden activations stay in registers. */
int di2p_point_chain(const di2p_src_t* srcs_host, int n_src, const float* W0t, int K0, const di2p_epilogue_t* epi0_host,
                     const float* W1t, const float* scale1, const float* shift1, int relu1, const float* W2t,
                     const float* scale2, const float* shift2, int relu2, float* Y, int B, int M, int N, void* stream);

int di2p_batch_gemv(const float* Wt, int M, int k0, const float* v, int Kv, float* out, int B, void* stream);
/* Two broadcast inputs in one launch: Y[b,m] = (sum_k Wt[k0+k,m] v0[b,k]) + (sum_k Wt[k1+k,m] v1[b,k]), each sum formed
 * exactly as di2p_batch_gemv forms it (node_b_pn: global PC feature + global image feature, networks_united.py:152-155). */
int di2p_batch_gemv2(const float* Wt, int M, int k0, const float* v0, int Kv0, int k1, const float* v1, int Kv1,
                     float* out, int B, void* stream);

/* Batched attention contraction of networks_united.py:147-150,170-174:
 * out[b,c,m] = (1/HW) * sum_hw feat[b,c,hw] * score[b,hw,m]. */
int di2p_attention_pool(const float* feat, const float* score, float* out, int B, int C, int HW, int Mn, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Image branch: ResNet-34 of models/resnet.py:56-72,125-216 (BasicBlock conv-bn-relu, residual
 * add, 7x7/2 stem, 3x3/2 max-pool, global average pool) as implicit-GEMM convolutions on fp32
 * MFMA with the BN(eval)+residual+ReLU epilogue fused.
 *   x f32[B,Cin,H,W] (NCHW), Wt f32[Cin*KH*KW, Cout] (weight[co,ci,kh,kw] transposed), y
 *   f32[B,Cout,OH,OW];  y = relu?( scale*conv(x) + shift + residual ).
 *   tap_major != 0: Wt rows are ordered (kh,kw,ci) instead of the weight's own (ci,kh,kw); needs Cin % 16 == 0 and
 *   lets the loader decode the filter tap once per 16-row K-step. */
int di2p_conv2d(const float* x, const float* Wt, const float* scale, const float* shift,
                const float* residual, float* y, int B, int Cin, int H, int W, int Cout,
                int KH, int KW, int stride, int pad, int relu, int tap_major, void* stream);
/* Same, with scratch for split-K: layers with few output pixels (ResNet stage 4) are cut into K-slices along the
 * filter taps, the partial sums (slices x B*Cout*OH*OW floats) are combined in slice order by a second pass.
 * di2p_conv2d_workspace_bytes returns the size this shape wants (0: no split); a NULL / too small workspace
 * silently runs unsplit.  Results are deterministic either way. */
int di2p_conv2d_ws(const float* x, const float* Wt, const float* scale, const float* shift,
                   const float* residual, float* y, int B, int Cin, int H, int W, int Cout,
                   int KH, int KW, int stride, int pad, int relu, int tap_major,
                   void* workspace, long long workspace_bytes, void* stream);
long long di2p_conv2d_workspace_bytes(int B, int Cin, int H, int W, int Cout, int KH, int KW, int stride, int pad,
                                      int tap_major);
/* 3x3 / stride 1 / pad 1 convolutions (26 of the 36 of ResNet-34, models/resnet.py:56-72) as a fused Winograd F(2x2,3x3) kernel:
 * 16 multiplications per 2x2 output tile and (ci, co) pair instead of 36; exact in exact arithmetic.
 *   di2p_winograd_weight_transform: weight f32[Cout,Cin,3,3] -> U f32[16,Cin,Cout] (= G g G^T), once per checkpoint load.
 *   di2p_conv3x3_winograd: y = relu?( scale * conv(x) + shift + residual ); needs Cin % 8 == 0 and Cout % 32 == 0. */
int di2p_winograd_weight_transform(const float* weight, float* U, int Cin, int Cout, void* stream);
/* round 6 (training path): the transformed filter of the INPUT GRADIENT of a stride-1 3x3 layer, U f32[16,Cin_g,Cout_g], straight from the layer's
 * forward filter weight f32[Cout_f = Cin_g, Cin_f = Cout_g, 3, 3] (taps flipped, channel roles swapped).  Replaces torch's flip + transpose + copy
 * in front of di2p_winograd_weight_transform (models/multimodal_classifier.py:213-218 reaches it through loss.backward()). */
int di2p_winograd_weight_transform_dgrad(const float* weight, float* U, int Cin_g, int Cout_g, void* stream);
int di2p_conv3x3_winograd(const float* x, const float* U, const float* scale, const float* shift, const float* residual, float* y, int B,
                          int Cin, int H, int W, int Cout, int relu, void* stream);
/* Routing queries of the fp32-MFMA inference family (additive; detect by symbol): which kernel instance a call would launch -- host code, each
 * launch entry's own routing function, nothing is launched and no device is needed (for tests and tools).  Each honours the knobs its entry
 * reads.  0 on success, -1 (di2p_last_error) on sizes the entry itself refuses.
 *   di2p_pointwise_route (di2p_pointwise_gemm; knobs pw_novec, conv_depth1).  dense: every source is DI2P_SRC_DENSE with row_stride % 4 == 0,
 *     batch_stride % 4 == 0 and a 16-byte aligned base; wt_aligned: Wt 16-byte aligned.
 *     out[0..5] = stager (0 scalar, 1 16-byte), tile rows, tile columns, dense loader, prefetch depth (1 / 2), K-step.
 *   di2p_conv2d_route (di2p_conv2d / _ws; knobs conv_nosplit, conv_s2scalar, conv_depth1).  x_aligned / wt_aligned: x / Wt 16-byte aligned;
 *     workspace_bytes: size of a 16-byte aligned workspace, 0 for none.
 *     out[0..6] = kernel (0 scalar stager, 1 16-byte stager, 2 the 7x7/2 row-decoding stager), tile rows, tile columns, K-step, stride
 *     variant (0 n/a, 1, 2, 22 = stride 2 through aligned 8-float windows), prefetch depth, K-slices actually used (1: no split-K).
 *   di2p_winograd_route (di2p_conv3x3_winograd; knobs wino_cob, wino_kc, wino_reg).
 *     out[0..7] = kernel (0 LDS-panel, 1 register-resident), output channels per workgroup, K-step (0: register-resident), waves, tile
 *     blocks, tiles per block, co-blocks, workgroups.
 *   di2p_point_chain_route (di2p_point_chain) on a device of `cus` compute units (the launch passes its own count).  layers: 2 or 3.
 *     out[0..7] = M, K-step of layer 0, layers, 32-column blocks per wave trip, nblk (trips per frame), total (trips), wgs (workgroups of
 *     4 waves), workgroups per compute unit.
 *   di2p_point_head_route (di2p_point_head; knob head_reg) on `cus` compute units.  c0: channels of source 0; reg_range: every source's
 *     channels * row_stride * 4 < 2^31; g33: both gathered tables given with k = 3.
 *     out[0..5] = kernel (0 LDS-tile, 1 wave-autonomous), G33 epilogue, columns per block, nblk (blocks per frame), total, wgs. */
int di2p_pointwise_route(int M, int K, int N, int B, int dense, int wt_aligned, int32_t* out);
int di2p_conv2d_route(int B, int Cin, int H, int W, int Cout, int KH, int KW, int stride, int pad, int tap_major, int x_aligned,
                      int wt_aligned, long long workspace_bytes, int32_t* out);
int di2p_winograd_route(int B, int Cin, int H, int W, int Cout, int32_t* out);
int di2p_point_chain_route(int M, int K0, int layers, int B, int N, int cus, int32_t* out);
int di2p_point_head_route(int K0, int n_src, int c0, int reg_range, int g33, int B, int N, int cus, int32_t* out);
/* The coarse per-point head (per_point_pn, models/networks_united.py:57-74 applied at :188-197: 736 -> 128 -> 128 -> P) in ONE launch on the bf16
 * matrix instructions with exact three-way fp32 splits, wave-autonomous (a wave keeps all 128 channels of 32 points in registers through the three
 * layers).  Layer 0 = the dense channels of the point (two sources f32[B, ch, N], channels multiples of 16) through W0 PLUS the per-node products
 * of its interpolated inputs, gathered from two node-major tables f32[B, nodes, 128] (3 neighbours each, idx i32[B,N,3], weights f32[B,N,3] or NULL
 * = 1) -- the same decomposition as di2p_point_head.  Weights: di2p_head_x3_pack of the [K][128] k-major matrices of layer 0 (rows of the dense
 * sources only) and layer 1; scale_shift = f32[4][128] (scale0, shift0, scale1, shift1); W2t f32[128][P], scale2 / shift2 f32[P] or NULL.
 * out f32[B,P,N].  This build runs 32 + 64 dense channels (K0 = 96), P <= 4; anything else: di2p_point_head / di2p_pointwise_gemm. */
typedef struct {
    const float* src[2]; long long batch_stride[2]; int row_stride[2]; int channels[2];
    const void* W0p; const void* W1p; const float* scale_shift; int relu0, relu1;
    const float* tab[2]; const int32_t* idx[2]; const float* w[2]; int nodes[2];
    const float* W2t; const float* scale2; const float* shift2; int relu2, P;
} di2p_head_x3_t;
long long di2p_head_x3_packed_bytes(int K);
int di2p_head_x3_pack(const float* Wt, int K, void* Wp, void* stream);
int di2p_point_head_x3(const di2p_head_x3_t* h, float* out, int B, int N, void* stream);
/* The labels-only tail of the FINE per-point head (per_point_pn of fine models, 736 -> 256 -> 256 -> P = 2 + L; the two argmaxes of
 * models/multimodal_classifier.py:100-117) in ONE launch on the bf16 matrix instructions with exact three-way fp32 splits:
 *   y1 = relu?(scale1 * W1 y0 + shift1);  s = scale2? * W2 y1 + shift2?;  coarse = argmax(s[0:2]), fine = argmax(s[2:P])  (int32 [B,N])
 * y0 = layer 0's output f32[B, K, N] (row stride >= N, batch stride >= K * row stride); this build runs K = 256 and any P >= 3.  Weights:
 * di2p_head_labels_x3_pack of W1t f32[K][K] and of W2t f32[K][P] (k-major; di2p_head_labels_x3_packed_bytes(K, M) bytes each, 16-byte aligned);
 * scale1 / shift1 f32[K] (required), scale2 / shift2 f32[P] or NULL.  scores: f32[B,P,N] or NULL (no score tensor is written).  Argmax
 * semantics of di2p_argmax_channels on the same scores: the first maximum wins, NaN ranks above everything (the first NaN wins). */
typedef struct {
    const float* y0; long long batch_stride; int row_stride; int K;
    const void* W1p; const float* scale1; const float* shift1; int relu1;
    const void* W2p; const float* scale2; const float* shift2; int P;
    float* scores; int32_t* coarse; int32_t* fine;
} di2p_head_labels_x3_t;
long long di2p_head_labels_x3_packed_bytes(int K, int P);
int di2p_head_labels_x3_pack(const float* Wt, int K, int P, void* Wp, void* stream);
int di2p_point_head_labels_x3(const di2p_head_labels_x3_t* h, int B, int N, void* stream);
/* 3x3 convolutions (pad 1, stride 1 or 2) on the bf16 matrix instructions with the EXACT three-way fp32 split of both operands ("bf16x3",
 * see di2p_pointwise_gemm_x3): a direct implicit GEMM whose input patch is split once while it is staged into LDS and then serves all nine
 * taps.  Replaces cuDNN's conv+BN+ReLU(+residual) of models/resnet.py:56-72 (BasicBlock.forward) for the layers it supports; with stride 2
 * the BasicBlock's 1x1 / stride-2 downsample branch (models/resnet.py:160-164, applied at :62-63) is computed from the same staged patch.
 *   Wp    = di2p_bf16x3_pack of the tap-major matrix Wt[(kh*3+kw)*Cin + ci][Cout] (K = 9 Cin, M = Cout);
 *   Wp_ds = di2p_bf16x3_pack of Wt_ds[Cin][Cout] (stride 2: required; stride 1: must be NULL);
 *   y     f32[B,Cout,OH,OW] = relu?(scale * conv3x3(x f32[B,Cin,H,W]) + shift + residual);  y_ds = scale_ds * conv1x1/s2(x) + shift_ds.
 *   cfg   = the tile configuration: 0..3 forces one, -1 takes the knob "conv_x3_cfg" (whose default -1 is the cheapest by a cost model).
 * di2p_conv3x3_x3_supported: 1 if a kernel instance of configuration cfg exists for the shape (OW % 32 == 0 and Cin % 16 == 0, or
 * OW % 16 == 0 and Cin % 32 == 0; the input patch of a tile must fit the LDS), else 0 -- the caller then uses di2p_conv3x3_winograd /
 * di2p_conv2d.  (ABI 8: cfg added to both.)
 * di2p_conv3x3_x3_plan (additive, ABI 9; detect by symbol): which kernel instance the call would run (host code, launches nothing; for
 * tests and tools: tests/conv_x3_cases.py keeps one layer shape per instance by it).  0 where
 * di2p_conv3x3_x3_supported is 0, else 1 and out[0..13] = configuration, instance index, instance count, fallback to the single-buffered
 * instance taken (0/1), double-buffered (0/1), staging items the plan needs, items of the instance, the instance's compile-time patch row
 * length (0: run-time), workgroup tiles per frame, Cout tiles, most output rows under one tile, nseg % NSEG (segments in the ragged last
 * tile, 0: none), Cout % MT (rows of the partial Cout tile, 0: none), Cin / KS (chunks of the K loop). */
int di2p_conv3x3_x3_supported(int B, int Cin, int H, int W, int Cout, int stride, int cfg);
int di2p_conv3x3_x3_plan(int B, int Cin, int H, int W, int Cout, int stride, int cfg, int32_t* out);
int di2p_conv3x3_x3(const float* x, const void* Wp, const float* scale, const float* shift, const float* residual, float* y, int B,
                    int Cin, int H, int W, int Cout, int stride, int relu, const void* Wp_ds, const float* scale_ds,
                    const float* shift_ds, float* y_ds, int cfg, void* stream);
/* The ResNet stem (7x7 / stride 2 / pad 3, 3 -> 64 channels, models/resnet.py:137-139,197-199) as a direct kernel: the filter bank and
 * the input row segments of a workgroup are staged once (columns de-interleaved by parity), then 168 MFMAs per wave without a barrier.
 *   di2p_stem_pack: weight f32[64,3,7,7] -> Wp f32[168,64] (taps padded 7 -> 8 per row), once per checkpoint load.
 *   di2p_conv7x7s2_stem: y f32[B,64,OH,OW] = relu?(scale * conv(x f32[B,3,H,W]) + shift). */
int di2p_stem_pack(const float* weight, float* Wp, void* stream);
int di2p_conv7x7s2_stem(const float* x, const float* Wp, const float* scale, const float* shift, float* y, int B, int H, int W, int relu,
                        void* stream);
int di2p_maxpool3x3s2(const float* x, float* y, int B, int C, int H, int W, void* stream);
/* The same head of the image branch -- conv1 7x7/2 + bn1 + relu + maxpool 3x3/2 (models/resnet.py:137-141,197-201) -- as ONE launch on the
 * bf16 matrix instructions with exact three-way fp32 splits (six bf16 products per fp32 product, fp32 accumulation: as accurate against fp64
 * as the fp32-MFMA stem); the 64 x H/2 x W/2 activation between the convolution and the pool stays in the compute unit.
 *   di2p_stem_x3_pack: weight f32[64,3,7,7] -> Wp (di2p_stem_x3_packed_bytes() bytes, 16-byte aligned), once per checkpoint load.
 *   di2p_stem_x3_supported: 1 if the image size runs (H % 4 == 0, W % 128 == 0, W <= 512), else 0 -- the caller then uses the two launches above.
 *   di2p_stem_x3: y f32[B,64,H/4,W/4] = maxpool3x3/2/pad1(relu(scale * conv7x7/2/pad3(x f32[B,3,H,W]) + shift)). */
long long di2p_stem_x3_packed_bytes(void);
int di2p_stem_x3_pack(const float* weight, void* Wp, void* stream);
int di2p_stem_x3_supported(int H, int W);
int di2p_stem_x3(const float* x, const void* Wp, const float* scale, const float* shift, float* y, int B, int H, int W, void* stream);
int di2p_global_avgpool(const float* x, float* y, int B, int C, int HW, void* stream);
/* out[b,c] = max_n x[b,c,n]  (networks_pc.py:115) */
int di2p_channel_max(const float* x, float* y, int B, int C, int N, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Registration: replaces evaluation/frustum_reg (registration.cpp:9-186 solvePGivenK, bound at
 * :190-206) + Ceres, and the 60-restart process fan-out of evaluation/registration_lsq.py:142-186.
 *
 * di2p_initial_guess: registration_lsq.py:196-220 on device.  points f64[F,3,N], labels
 *   i32[F,N] -> yaw0 f64[F]; labels_out i32[F,N] = label, or -1 for points removed by the front
 *   filter (the solver skips labels not in {0,1}, registration.cpp:87-125); has_inside i32[F].
 * di2p_solve_batched: F frames x R hypotheses.  One 4-wavefront workgroup per hypothesis; Cauchy-robust
 *   Levenberg-Marquardt with box bounds on t (see DESIGN.md for the exact algorithm statement).
 *   points f64[F,3,N], labels i32[F,N], K f64[F,3,3] (fx,fy,cx,cy used), init_y f64[F,R],
 *   init_T f64[F,R,3], lb/ub f64[3] HOST arrays, is_2d: 4 params [ry,tx,ty,tz] else 6
 *   [angle-axis, t].  Outputs: params f64[F,R,np], cost f64[F,R], iters i32[F,R], sweeps i32[F,R] (optional).
 *   If yaw0 != NULL it is added to init_y per frame (restart noise drawn before yaw0 is known).
 *   A hypothesis whose (box-projected) start cannot be evaluated -- a non-finite residual or Jacobian entry -- returns that start with
 *   iters 0 and cost NaN, which di2p_select_best never selects.
 *   workspace: di2p_solve_workspace_bytes(F, R, N) bytes of scratch (sorted point records, cluster boxes, sort keys,
 *   parked Levenberg-Marquardt states of the two-tier launch).
 * di2p_select_best: argmin cost over R per frame (ties -> lowest r; frames with has_inside==0 get
 *   identity and cost 1e4, registration_lsq.py:329-332) -> best i32[F], P f64[F,4,4], cost f64[F].
 * di2p_solver_residuals: Problem::Evaluate of registration.cpp:150-155 at given params:
 *   loss-corrected residuals in point order (3 per label-1 point, 1 per label-0 point), compacted
 *   per frame into residuals f64[F, 3N] with counts i32[F]; cost f64[F]. */
int di2p_initial_guess(const double* points, const int32_t* labels, double* yaw0, int32_t* labels_out,
                       int32_t* has_inside, int F, int N, void* stream);
int di2p_solve_batched(const double* points, const int32_t* labels, const double* K,
                       const double* init_y, const double* init_T, const double* yaw0,
                       double H, double W, const double* lb_host, const double* ub_host,
                       int max_iter, int is_2d, int F, int R, int N,
                       double* params, double* cost, int32_t* iters, int32_t* sweeps /* may be NULL: #passes over the points */, void* workspace, void* stream);
/* Same solver reading the points as f32 [F,3,N] (the network's own pc tensor; widening to f64 is
 * exact, so results are bit-identical to di2p_solve_batched on the widened copy). */
int di2p_solve_batched_f32(const float* points, const int32_t* labels, const double* K,
                           const double* init_y, const double* init_T, const double* yaw0,
                           double H, double W, const double* lb_host, const double* ub_host,
                           int max_iter, int is_2d, int F, int R, int N,
                           double* params, double* cost, int32_t* iters, int32_t* sweeps /* may be NULL: #passes over the points */, void* workspace, void* stream);
long long di2p_solve_workspace_bytes(int F, int R, int N);
/* diagnostics only: device buffer of F*R*28 int64 (or NULL) receiving per-hypothesis phase cycle counts and cluster statistics
 * (layout: csrc/solver.hip at the definition; F*R*8 words up to version 2, 16 in version 3, 20 in versions 4-5).  While set, solves run
 * a separate, instrumented kernel. */
void di2p_solver_set_profile_buffer(void* buf);
int di2p_select_best(const double* params, const double* cost, const int32_t* has_inside, int is_2d,
                     int F, int R, int32_t* best, double* P, double* best_cost, void* stream);
int di2p_solver_residuals(const double* points, const int32_t* labels, const double* K,
                          const double* params, double H, double W, int is_2d, int F, int N,
                          double* residuals, int32_t* counts, double* cost, void* stream);

/* ---------------------------------------------------------------------------------------------
 * "Next" rows: the steps directly before and after the classifier.
 * di2p_farthest_point_sampling: FarthestSampler.sample of data/kitti_helper.py:224-243 (called at
 *   data/kitti_pc_img_pose_loader.py:416-423).  pts f32[B,3,M] (M <= 4096 candidate points), init_idx i32[B] or
 *   NULL (= 0; the reference draws randint(len(pts)) = randint(3)) -> idx i32[B,k], nodes f32[B,3,k] (may be NULL).
 *   numpy semantics: fp64 squared distances, np.minimum update, first-occurrence argmax.
 * di2p_gather_points: out[b,c,n] = src[b,c,idx[b,n]] -- the down-sampling of kitti_pc_img_pose_loader.py:158-171
 *   with the host-drawn index list as an explicit input.
 * di2p_project_labels: evaluation/visualize_and_save_data.py:100-115,138-139 (same arithmetic as
 *   models/multimodal_classifier.py:135-156): P f32[B,p_rows(3|4),4], K f32[B,3,3] -> coarse i32[B,N] (inside-frustum,
 *   <= W-1, z > 0.1), fine i32[B,N] = floor(px/scale) + floor(py/scale)*W_fine (may be NULL), pxpy f32[B,2,N] (may be NULL).
 * di2p_label_accuracy: :142-145 -> out f32[B,2] = {coarse accuracy, fine accuracy over gt-inside points (NaN if none)}.
 * di2p_pack_pc_label: the 7 x N hand-off record of :174-181 (xyz, coarse_pred, coarse_gt, fine_pred, fine_gt) as
 *   f64[B,7,N], i.e. what np.load(..._pc_label.npy) gives evaluation/registration_lsq.py:291-296. */
int di2p_farthest_point_sampling(const float* pts, const int32_t* init_idx, int32_t* idx_out, float* nodes_out,
                                 int B, int M, int k, void* stream);
int di2p_gather_points(const float* src, const int32_t* idx, float* out, int B, int C, int Nsrc, int Nout, void* stream);
int di2p_project_labels(const float* pc, const float* P, int p_rows, const float* K, float H, float W, float fine_scale,
                        int32_t* coarse, int32_t* fine, float* pxpy, int B, int N, void* stream);
int di2p_label_accuracy(const int32_t* coarse_pred, const int32_t* coarse_gt, const int32_t* fine_pred,
                        const int32_t* fine_gt, float* out, int B, int N, void* stream);
int di2p_pack_pc_label(const float* pc, const int32_t* coarse_pred, const int32_t* coarse_gt, const int32_t* fine_pred,
                       const int32_t* fine_gt, double* out, int B, int N, void* stream);

/* ---------------------------------------------------------------------------------------------
 * PnP back end of config 3 -- replaces cv2.solvePnPRansac as called by evaluation/registration_pnp.py:95-148
 * (solve_PnP).  OpenCV is absent (parity unpinned): the algorithm is stated in csrc/pnp.hip and DESIGN.md.
 *   pc f32[F,3,N], coarse i32[F,N] (1 = use the point), fine i32[F,N] (cell id: pixel = (fine % W_fine, fine / W_fine))
 *   or explicit pixels f32[F,2,N] (then fine may be NULL), K_scaled f64[F,3,3] (already multiplied by the 1/32 scale,
 *   camera_matrix_scaling :58-61), samples i32[F,iters,6] (RANSAC draws, taken modulo the frame's correspondence count),
 *   reproj_err in scaled pixels (reference: 0.6); local optimisation of the best model: refine_rounds rounds of
 *   {re-estimate inliers, refine_iters Gauss-Newton steps}, a round kept only if it loses no inliers.
 *   -> P f64[F,4,4] (identity when rejected), outlier_ratio f64[F] (1 when rejected), n_inliers, n_corr, best i32[F].
 *   workspace: di2p_pnp_workspace_bytes(F, N, iters).
 *   Both RANSAC entry points lay the workspace out the same way, each region starting where the one before it ends, rounded up to 256 bytes:
 *     corr    f32[F][N][8]       the packed correspondences {x, y, z, u, v, 0, 0, 0}, the first n_corr[f] records of frame f valid
 *     hyp     f64[F][iters][13]  per hypothesis R (9, row-major), t (3), valid flag (0 / 1); R and t are undefined where the flag is 0
 *     inliers i32[F][iters]      per-hypothesis inlier count, -1 for an invalid hypothesis
 *     mask    u8[F][N]           the inlier mask over the frame's records: of the winning hypothesis (EPnP), of the model the last
 *                                refinement round started from (DLT); written for frames with a model only
 *   The regions are READABLE AFTER THE CALL, for tests and debugging (deepi2p_amd/registration_pnp.py: workspace_views); nothing outside
 *   them is defined, and the end of `mask` lies within di2p_pnp_workspace_bytes(F, N, iters). */
long long di2p_pnp_workspace_bytes(int F, int N, int iters);
/* The correspondence list alone: what solve_PnP (evaluation/registration_pnp.py:97-110) hands to cv2.solvePnPRansac (:125-127) -- points =
 * pc[:, coarse == 1], pixels = (fine - floor(fine / W) * W, floor(fine / W)), in point order.  corr f32[F][N][8] = {x, y, z, u, v, 0, 0, 0},
 * the first n_corr[f] records of frame f valid.  (The RANSAC entry points below pack internally; this one exists so the packing can be
 * compared with what the reference's own function passes to OpenCV: tests/golden/pnp_frontend_golden.npz.) */
int di2p_pnp_pack(const float* pc, const int32_t* coarse, const int32_t* fine, const float* pixels, int W_fine, int F, int N,
                  float* corr, int32_t* n_corr, void* stream);
int di2p_pnp_ransac(const float* pc, const int32_t* coarse, const int32_t* fine, const float* pixels,
                    const double* K_scaled, int W_fine, const int32_t* samples, int iters, double reproj_err,
                    int refine_rounds, int refine_iters, int F, int N, double* P_out, double* outlier_ratio, int32_t* n_inliers,
                    int32_t* n_corr, int32_t* best, void* workspace, void* stream);
/* The estimator the reference names (flags = cv2.SOLVEPNP_EPNP, evaluation/registration_pnp.py:125-132): EPnP on minimal
 * samples of 5 correspondences (the first 5 entries of each row of `samples`; 4 when the frame has only 4), inlier iff the squared
 * reprojection error <= reproj_err^2, the model with the most inliers, one EPnP re-fit on all of its inliers; frames with
 * fewer than 4 correspondences or no model are rejected (identity, outlier ratio 1).  Same buffers as di2p_pnp_ransac. */
int di2p_pnp_ransac_epnp(const float* pc, const int32_t* coarse, const int32_t* fine, const float* pixels,
                         const double* K_scaled, int W_fine, const int32_t* samples, int iters, double reproj_err, int F, int N,
                         double* P_out, double* outlier_ratio, int32_t* n_inliers, int32_t* n_corr, int32_t* best,
                         void* workspace, void* stream);

/* f32 -> f64 widening copy of the point cloud for the solver ([B,3,N]) and i32 label passthrough
 * are done by the caller; helper for the fused pipeline: */
int di2p_f32_to_f64(const float* in, double* out, long long n, void* stream);

/* ---- on-device random draws (counter-based Philox4x32-10: every value is a function of (seed, index) only) -------------
 * di2p_draw_restarts: the solver's restart list (evaluation/registration_lsq.py:163-164): ry_noise f64[F,R] ~ N(0, ry_sigma)
 *   (the frame's yaw0 is added by the solver), init_T f64[F,R,3] = (0, 0, U(-t_amplitude, t_amplitude)).
 * di2p_random_choice: n_out of n_src indices without replacement, in random order, per frame
 *   (np.random.choice(n_src, n_out, replace=False) of data/kitti_pc_img_pose_loader.py:158-171,416-423);
 *   stream_id separates independent draws under one seed; workspace: di2p_random_choice_workspace_bytes(B, n_src). */
int di2p_draw_restarts(unsigned long long seed, int F, int R, double ry_sigma, double t_amplitude, double* ry_noise,
                       double* init_T, void* stream);
long long di2p_random_choice_workspace_bytes(int B, int n_src);
int di2p_random_choice(unsigned long long seed, int stream_id, int B, int n_src, int n_out, int32_t* idx_out, void* workspace,
                       void* stream);

/* (additive, after ABI 7) di2p_random_choice_ragged: the same draw per frame with n_src = offsets[b+1] - offsets[b] read on the device (<= max_src, the
 *   caller's per-frame capacity): frame b equals di2p_random_choice's frame b for that n_src; a frame shorter than n_out takes every index
 *   floor(n_out / n_src) times, then the first n_out mod n_src of its draw (prep.downsample's rule); an empty frame gives -1.
 *   workspace: di2p_random_choice_ragged_workspace_bytes(B, max_src). */
long long di2p_random_choice_ragged_workspace_bytes(int B, int max_src);
int di2p_random_choice_ragged(unsigned long long seed, int stream_id, int B, const int32_t* offsets, int max_src, int n_out, int32_t* idx_out,
                              void* workspace, void* stream);

/* ---- (additive, after ABI 7; detect by symbol) raw LiDAR scan preparation (csrc/scan_prep.hip) -------------------------------------------------------------------
 * Replaces data/kitti/kitti_pc_bin_to_npy_with_downsample_sn.py:50-74 (Open3D voxel_down_sample, estimate_normals with a hybrid
 * radius / max_nn search, orient_normals_to_align_with_direction([0,0,1]), cKDTree 1-NN intensity) and the loader's second voxel pass
 * and random down-sample (data/kitti_pc_img_pose_loader.py:26-44,158-171,296-306,380).
 * A batch is ragged: points f32[total,4] (KITTI .bin rows x, y, z, intensity), offsets i32[B+1] (device, offsets[0] = 0), cap >= total the
 * fixed capacity every per-point / per-output-point buffer is sized for.  Coordinates must be finite (non-finite input is outside the
 * contract).  Outputs are ragged too, with device offsets: out_offsets i32[B+1]; output point j of frame b is row out_offsets[b] + j.
 * ONE workspace of di2p_scan_prep_workspace_bytes(B, cap) bytes (256-byte aligned) carries a batch through the three calls, in order:
 * di2p_voxel_down_sample first, then di2p_estimate_normals and / or di2p_nearest_raw with the same B, cap and out_offsets.
 *
 * di2p_voxel_down_sample: Open3D VoxelDownSample, deterministic.  Per frame min_bound = min - voxel/2, voxel index floor((p - min_bound) /
 *   voxel) in fp64; one output point per occupied voxel in ascending (ix, iy, iz), the fp64 mean of its members summed in ascending input
 *   index; out_intensity = mean(i / max_frame(i)) * max_frame(i) (the loader's fake colour); out_normals (needs normals_in f32[total,3]) the
 *   plain mean, not renormalised; out_keys i64 = ix << 42 | iy << 21 | iz.  Frames with at most min_points points are copied unchanged
 *   (the loader's "> 2 * input_pt_num" rule; 0 = every frame is voxelised).  status i32[B] (may be NULL): 0 ok, 1 more than
 *   max_frame_points (<= 2^20) points, 2 a bounding-box edge above max_extent or a voxel index above 2^21 - 1, 3 bad offsets; such a
 *   frame has no output points.  max_extent / voxel must stay below 2^21 - 2.  out_intensity / out_normals / out_keys / status may be NULL.
 * di2p_estimate_normals: per output point of the voxel call, the <= max_nn (<= 64) nearest output points of its frame with d^2 < radius^2
 *   (fp64, the point itself included), the eigenvector of the smallest eigenvalue of their covariance, (0,0,1) for fewer than 3 neighbours
 *   or a zero covariance, flipped so that n_z >= 0.  normals f32[cap,3]; nn_count i32[cap] and nn_idx i32[cap,max_nn] (frame-local
 *   output indices by ascending (d^2, index), -1 padded) may be NULL.  max_extent / radius must stay below 2^21 - 4.
 * di2p_nearest_raw: per output point, the nearest raw point of its frame (exact fp64 d^2, ties -> lower index): nn_idx i32[cap]
 *   (frame-local raw index), nn_intensity f32[cap] its intensity, nn_dist2 f64[cap] (each may be NULL).  voxel as in the voxel call.
 * di2p_gather_ragged: out[b,:,n] = src[offsets[b] + idx[b,n]] for points f32[total,3] / intensity f32[total] / normals f32[total,3] into
 *   pc f32[B,3,n_out], intensity_out f32[B,1,n_out], sn f32[B,3,n_out]; idx < 0 gives zeros.  transform f64[B,4,4] (may be NULL): points
 *   by [R|t], normals by R, in fp64. */
long long di2p_scan_prep_workspace_bytes(int B, int cap);
int di2p_voxel_down_sample(const float* points, const int32_t* offsets, int B, int cap, int max_frame_points, double voxel, double max_extent,
                           int min_points, const float* normals_in, int32_t* out_offsets, float* out_points, float* out_intensity,
                           float* out_normals, int64_t* out_keys, int32_t* status, void* workspace, void* stream);
int di2p_estimate_normals(const int32_t* voxel_offsets, int B, int cap, double radius, int max_nn, double max_extent, float* normals,
                          int32_t* nn_count, int32_t* nn_idx, void* workspace, void* stream);
int di2p_nearest_raw(const float* points, const int32_t* offsets, const int32_t* voxel_offsets, int B, int cap, double voxel, int32_t* nn_idx,
                     float* nn_intensity, double* nn_dist2, void* workspace, void* stream);
int di2p_gather_ragged(const float* points, const float* intensity, const float* normals, const int32_t* offsets, const int32_t* idx,
                       const double* transform, int B, int n_out, float* pc, float* intensity_out, float* sn, void* stream);

/* ---- training-side head (losses and optimiser; the backward kernels follow below) ----------------
 * di2p_classifier_loss: the losses of models/multimodal_classifier.py:189-191 and d loss / d scores in one pass:
 *   coarse f32[B,2,N] with FocalLoss(alpha, gamma, 'mean') * coarse_loss_alpha (models/focal_loss.py:55-112), fine f32[B,L,N]
 *   (or NULL) with mean cross-entropy over the points whose coarse label is 1; labels i32[B,N] (di2p_project_labels).
 *   out8 f64[8] = {loss, coarse loss, fine loss, coarse accuracy, fine accuracy, inside count, 0, 0};
 *   d_coarse f32[B,2,N] / d_fine f32[B,L,N] (may be NULL: losses only).  workspace: di2p_classifier_loss_workspace_bytes(B, N).
 * di2p_adam_step: torch.optim.Adam (weight_decay 0, amsgrad off; :44-47) on one flat fp32 buffer, step counted from 1. */
long long di2p_classifier_loss_workspace_bytes(int B, int N);
int di2p_classifier_loss(const float* coarse, const float* fine, const int32_t* coarse_labels, const int32_t* fine_labels,
                         int B, int N, int L, float alpha, float gamma, float coarse_loss_alpha, double* out8,
                         float* d_coarse, float* d_fine, void* workspace, void* stream);
int di2p_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, long long n, int step, float lr,
                   float beta1, float beta2, float eps, void* stream);

/* ---- training: backward kernels and train-mode BatchNorm (replaces the torch.autograd backward of
 *      models/multimodal_classifier.py:213-218).  All tensors f32, [B,C,N] (or NCHW with N = H*W), contiguous. ----------------------
 * di2p_bn_train_forward: nn.BatchNorm1d/2d in train mode (layers_pc.py:283,150-160; resnet.py:44-70): batch mean / biased variance over
 *   (B,N), y = relu?((x-mean)*invstd*gamma + beta + residual?); running stats updated with `momentum` and the unbiased variance
 *   (running_* may both be NULL).  workspace: di2p_channel_reduce_workspace_bytes(B, C, N).
 * di2p_bn_train_backward: g = dy * [y > 0] (relu) ; dgamma = sum g*xhat, dbeta = sum g, dx = gamma*invstd*(g - mean g - xhat*mean(g*xhat)),
 *   dresidual = g (may be NULL).
 * di2p_channel_sum: out[c] = sum_{b,n} x[b,c,n] (bias gradients).
 * di2p_bmm_rc: out[z][row][col] = alpha * sum_r A[z][row*lda + r] * B[z][col*ldb + r]  (both operands contiguous along the reduction:
 *   d W[M][K] = sum_{b,n} dY[b][m][n] X[b][k][n] with reduce_z = 1; attention d feat with reduce_z = 0).  Deterministic chunked reduction;
 *   workspace: di2p_bmm_rc_workspace_bytes(Z, rows, cols, R).
 * di2p_rc_route / di2p_rc_vec_ok (additive; detect by symbol): which kernel instance and chunk plan a call of this family runs -- host code,
 *   the launcher's own routing function, launches nothing (for tests and tools).  kind 0 = di2p_bmm_rc, 1 = di2p_conv2d_wgrad (rows = Cout,
 *   cols = Cin*KH*KW, R = OH*OW, Z = B), 2 = di2p_gather_backward (rows = C, cols = M, R = J, Z = B); a_vec / b_vec = di2p_rc_vec_ok of the
 *   strided operand(s) (1: 16-byte aligned base, ld % 4 == 0, batch_stride % 4 == 0, R % 4 == 0, R >= 32; honours the knob "rc_tile64").
 *   out[0..4] = tile (64 or 128), A stager, B stager (0 scalar, 1 16-byte), reduction indices per chunk, chunks; the workspace the call
 *   needs is Z * chunks * rows * cols * 4 bytes.
 * di2p_bmm_km: out[z][row][col] = alpha * sum_k A[z][k*lda + row] * B[z][k*ldb + col]  (attention d score).
 * di2p_gather_backward: d feats[b,c,m] = sum_j dy[b,c,j] * sum_k w[b,j,k] * [idx[b,j,k] == m]; k = 1 (torch.gather along the point axis,
 *   weights NULL = 1) or k = 3 (upsample_by_interpolation, networks_united.py:90-103).  workspace: di2p_gather_backward_workspace_bytes.
 * di2p_conv2d_wgrad / di2p_conv2d_dgrad: gradients of nn.Conv2d (bias-free; resnet.py) w.r.t. weight[Cout][Cin][KH][KW] and input.
 * di2p_maxpool3x3s2_backward, di2p_segment_max_backward (index_max + gather + mask, networks_pc.py:88-93), di2p_group_max_forward /
 *   _backward (max over the last axis with its first arg-max): the gradient goes to the arg-max element.
 * di2p_dropout_mask / di2p_apply_mask: nn.Dropout keep-mask from the counter-based generator (a function of seed, stream_id, index)
 *   and y = mask ? x*scale : 0. */
long long di2p_channel_reduce_workspace_bytes(int B, int C, int N);
int di2p_bn_train_forward(const float* x, const float* gamma, const float* beta, const float* residual, float* y, float* save_mean,
                          float* save_invstd, float* running_mean, float* running_var, float momentum, float eps, int relu, int B, int C,
                          int N, void* workspace, void* stream);
int di2p_bn_train_backward(const float* x, const float* y, const float* dy, const float* gamma, const float* save_mean,
                           const float* save_invstd, int relu, float* dx, float* dresidual, float* dgamma, float* dbeta, int B, int C, int N,
                           void* workspace, void* stream);
int di2p_channel_sum(const float* x, float* out, int B, int C, int N, void* workspace, void* stream);
long long di2p_bmm_rc_workspace_bytes(int Z, int rows, int cols, int R);
int di2p_bmm_rc(const float* A, long long lda, long long a_batch_stride, const float* Bm, long long ldb, long long b_batch_stride, float* out,
                int Z, int rows, int cols, int R, float alpha, int reduce_z, void* workspace, long long workspace_bytes, void* stream);
int di2p_rc_vec_ok(const float* base, long long ld, long long batch_stride, int R);
int di2p_rc_route(int kind, int Z, int rows, int cols, int R, int a_vec, int b_vec, int32_t* out);
int di2p_bmm_km(const float* A, int lda, long long a_batch_stride, const float* Bm, int ldb, long long b_batch_stride, float* out, int Z,
                int rows, int cols, int K, float alpha, void* stream);
long long di2p_gather_backward_workspace_bytes(int B, int C, int J, int M);
int di2p_gather_backward(const float* dy, const int32_t* idx, const float* weights, int k, float* dfeats, int B, int C, int J, int M,
                         void* workspace, long long workspace_bytes, void* stream);
long long di2p_conv2d_wgrad_workspace_bytes(int B, int Cin, int H, int W, int Cout, int KH, int KW, int stride, int pad);
int di2p_conv2d_wgrad(const float* x, const float* dy, float* dW, int B, int Cin, int H, int W, int Cout, int KH, int KW, int stride, int pad,
                      void* workspace, long long workspace_bytes, void* stream);
int di2p_conv2d_dgrad(const float* dy, const float* Wgt, float* dx, int B, int Cin, int H, int W, int Cout, int KH, int KW, int stride, int pad,
                      void* stream);
int di2p_maxpool3x3s2_backward(const float* x, const float* dy, float* dx, int B, int C, int H, int W, void* stream);
int di2p_segment_max_backward(const float* dvalues, const int32_t* max_idx, const float* mask, float* dx, int B, int C, int N, int M,
                              void* stream);
int di2p_group_max_forward(const float* x, float* y, int32_t* arg, long long rows, int K, void* stream);
int di2p_group_max_backward(const float* dy, const int32_t* arg, float* dx, long long rows, int K, void* stream);
int di2p_dropout_mask(unsigned long long seed, int stream_id, float p, long long n, uint8_t* mask, void* stream);
int di2p_apply_mask(const float* x, const uint8_t* mask, float scale, float* y, long long n, void* stream);

/* ---- training-sample preparation (csrc/sample_prep.hip; data/kitti_pc_img_pose_loader.py:108-156,199-232,326-384,439) -------------
 * Everything here launches on `stream` without allocating or synchronising; B == 0 is a valid no-op.  Where a seed is taken, seed_dev
 * (one 64-bit word in device memory, may be NULL) overrides `seed` and is read when the kernel runs, so a captured graph can be replayed
 * with another seed.
 * di2p_sample_draws: per frame b (a pure function of (seed, frame0 + b); Philox stream tag 4), from raw K f64[B,3,3], Pc f64[B,4,4] and
 *   Pji f64[B,4,4] (NULL: identity):  ints i32[B,8] = {dx, dy, flip, op0, op1, op2, op3, hue shift}: the crop window (train: uniform in
 *   [0, Ws - img_W] x [0, Hs - img_H]; else centred), the flip bit (train: probability 1/2), the order of the colour operations
 *   (0 brightness, 1 contrast, 2 saturation, 3 hue; a uniform permutation) and uint8(hue * 255), computed from the fp64 hue factor: the
 *   image path reads the shift from ints[7] only, factors[3] (the factor rounded to float32) is informative and may give a shift one
 *   off at a truncation boundary;  factors f32[B,4] = brightness, contrast,
 *   saturation, hue (uniform in color_range; 1, 1, 1, 0 outside train mode);  Pr f64[B,4,4] (train: Rz Ry Rx of uniform angles and a uniform
 *   translation in +- amplitude, times diag(-1,1,1,1) when flipped; val_random_Ry: Ry in +- 2 pi whatever amplitude[4]; val: identity);  PrPcn = Pr . P_cam_nwu
 *   f64[B,4,4] (the transform of the point kernels);  P = Pji . Pc . P_nwu_cam . Pr^-1 f32[B,3,4] (fp64, closed-form rigid inverse, rounded
 *   once);  K_out f32[B,3,3] = K after crop-top, scale, crop-window (the flip does not touch K).
 * di2p_image_prepare: images u8[B,H0,W0,3] -> out f32[B,3,img_H,img_W] (integral values 0..255) from the draw tables: top-row crop, the
 *   rounded 2x2 mean (img_scale 0.5, even cropped source dimensions) or no resize (1.0), the crop window, the colour chain in the frame's
 *   order with PIL's arithmetic, the flip.  geometry = 0: the source already is img_H x img_W, no crop / resize / flip; color = 0: no colour
 *   chain.  reduce_blocks: workgroups per frame of the grey-sum launch (0: default; the sum is an integer, so any value gives the same bits).
 *   workspace: di2p_image_prepare_workspace_bytes(B); afterwards its first B uint32 hold the grey sums the contrast operation used.
 * di2p_transform_segments: points f32[total,4] (x, y, z, intensity) / normals f32[total,3] (may be NULL): segment s (rows seg_offsets[s] ..
 *   seg_offsets[s+1]) by transforms f64[S,4,4] (points [R|t], normals R; fp64, rounded once), in place or into a second buffer.
 * di2p_gather_ragged_aug: di2p_gather_ragged with clip(sigma * N(0,1), +-clip), rounded to float32, added to every gathered coordinate
 *   and normal component before the transform; normals take the ROTATION of the transform only (the reference's homogeneous transform
 *   would add a non-zero translation of Pr to them) (Philox stream tag 5; a function of (seed, stream_id, frame, output index, component)).
 * di2p_random_choice_dseed / _ragged_dseed: di2p_random_choice / _ragged with the seed read from device memory. */
typedef struct {
    int mode;               /* 0 train, 1 val, 2 val_random_Ry */
    int crop_top;           /* crop_original_top_rows */
    double img_scale;       /* 0.5 or 1.0 (the _ds entry points: any value in (0, 1], it scales K) */
    int img_H, img_W;       /* the crop window */
    int Hs, Ws;             /* the scaled image: (H0 - crop_top) * img_scale, W0 * img_scale */
    double amplitude[6];    /* P_tx, P_ty, P_tz, P_Rx, P_Ry, P_Rz */
    double color_range[8];  /* brightness, contrast, saturation, hue: lo, hi */
} di2p_sample_opt_t;
int di2p_sample_draws(unsigned long long seed, const unsigned long long* seed_dev, int B, int frame0, const di2p_sample_opt_t* opt,
                      const double* K, const double* Pc, const double* Pji, int32_t* ints, float* factors, double* Pr, double* PrPcn,
                      float* P, float* K_out, void* stream);
long long di2p_image_prepare_workspace_bytes(int B);
int di2p_image_prepare(const uint8_t* images, int B, int H0, int W0, const di2p_sample_opt_t* opt, const int32_t* ints,
                       const float* factors, int geometry, int color, int reduce_blocks, float* out, void* workspace, void* stream);
int di2p_transform_segments(const float* points, const float* normals, const int32_t* seg_offsets, const double* transforms, int S,
                            int total, float* points_out, float* normals_out, void* stream);
int di2p_gather_ragged_aug(const float* points, const float* intensity, const float* normals, const int32_t* offsets, const int32_t* idx,
                           const double* transform, int B, int n_out, unsigned long long seed, const unsigned long long* seed_dev,
                           int stream_id, double sigma, double clip, float* pc, float* intensity_out, float* sn, void* stream);
int di2p_random_choice_dseed(const unsigned long long* seed_dev, int stream_id, int B, int n_src, int n_out, int32_t* idx_out,
                             void* workspace, void* stream);
int di2p_random_choice_ragged_dseed(const unsigned long long* seed_dev, int stream_id, int B, const int32_t* offsets, int max_src,
                                    int n_out, int32_t* idx_out, void* workspace, void* stream);

/* ---- (additive, ABI 9; detect by symbol) sample preparation of the Oxford and nuScenes loaders (data/oxford_pc_img_pose_loader.py:220-380,
 *      data/nuscenes_pc_img_pose_loader.py:213-267,273-408).  Same conventions as above: asynchronous, capturable, seed or *seed_dev. ----
 * di2p_range_shuffle (csrc/scan_prep.hip): ragged range filter + shuffle + compaction of the Oxford loader (:269-279), one call per batch.
 *   Point i of frame b is kept iff fl32(fl32(x x) + fl32(z z)) < fl32(r r) with r = (float)max_range (strict; max_range <= 0 keeps all).  The kept
 *   points of a frame come out in ascending order of key(seed, b, i) = (w0 << 32 | w1) >> 1 of Philox counter (i, b, 0, 6) -- stream tag 6, used
 *   by nothing else -- ties to the lower i.  out_points f32[cap,4], out_offsets i32[B+1]; a frame may keep nothing.  status i32[B] (may be
 *   NULL): 0 ok, 1 more than max_frame_points (<= 2^20) points, 3 bad offsets; such a frame has no output rows and nothing is written for
 *   it.  workspace: di2p_scan_prep_workspace_bytes(B, cap), 256-byte aligned; it may be the one di2p_voxel_down_sample uses afterwards.
 * di2p_gather_ragged_aug_intensity: di2p_gather_ragged_aug without normals, and with the same clipped noise additionally added to the
 *   intensity (float32 + float32) from Philox component slot DI2P_JITTER_SLOT_INTENSITY, which di2p_gather_ragged_aug leaves unused
 *   (0..2 the coordinates, 4..6 the normal).  The coordinate noise is di2p_gather_ragged_aug's, bit for bit.
 * di2p_sample_draws_ds: di2p_sample_draws for dataset 1 (Oxford) / 2 (nuScenes).  The uniforms of the frame keep their meaning (window,
 *   order, factors, translations, angles); no flip is drawn (ints[2] = 0); color_enable i32[B] = (u > 0.5) of one further uniform of the
 *   frame (Philox block 7; 0 outside train mode);  Pr f64[B,4,4] = [Rz Ry Rx | t] from all six amplitudes, applied by the point kernels to the
 *   cloud in the frame it is stored in;  val_random_Ry: +- 2 pi about y (Oxford) / about z (nuScenes);  P = P_cam_pc . Pr^-1 f32[B,3,4]
 *   (fp64, closed-form rigid inverse, rounded once);  K_out = K after crop-top (0 for Oxford: the bottom crop does not move K), scale,
 *   crop-window;  t_ij f32[B,3] = P_cam_pc[:3,3] (may be NULL).  opt->img_scale may be any value in (0, 1] here.
 * di2p_image_prepare_ds: di2p_image_prepare with crop_bottom rows removed below, resize_k (0: opt->img_scale 0.5 / 1.0 as above; odd k >= 3
 *   dividing both cropped source dimensions: output pixel (y, x) is the source pixel (k y + (k-1)/2, k x + (k-1)/2), which is INTER_LINEAR at
 *   scale 1/k with an explicit dsize -- derived from OpenCV's coordinate rule, not checked against OpenCV), color_enable i32[B] (NULL: every
 *   frame) gating the colour chain per frame, and no flip whatever ints[2] holds.  opt->Hs / Ws: the cropped source size over k. */
#define DI2P_JITTER_SLOT_INTENSITY 3
int di2p_range_shuffle(const float* points, const int32_t* offsets, int B, int cap, int max_frame_points, double max_range,
                       unsigned long long seed, const unsigned long long* seed_dev, float* out_points, int32_t* out_offsets, int32_t* status,
                       void* workspace, void* stream);
int di2p_gather_ragged_aug_intensity(const float* points, const float* intensity, const int32_t* offsets, const int32_t* idx,
                                     const double* transform, int B, int n_out, unsigned long long seed, const unsigned long long* seed_dev,
                                     int stream_id, double sigma, double clip, float* pc, float* intensity_out, void* stream);
int di2p_sample_draws_ds(unsigned long long seed, const unsigned long long* seed_dev, int B, int frame0, const di2p_sample_opt_t* opt,
                         int dataset, const double* K, const double* P_cam_pc, int32_t* ints, float* factors, int32_t* color_enable,
                         double* Pr, float* P, float* K_out, float* t_ij, void* stream);
int di2p_image_prepare_ds(const uint8_t* images, int B, int H0, int W0, const di2p_sample_opt_t* opt, int crop_bottom, int resize_k,
                          const int32_t* ints, const float* factors, const int32_t* color_enable, int color, int reduce_blocks, float* out,
                          void* workspace, void* stream);

/* ---- (additive, ABI 9; detect by symbol) raw frames in one call: cell-cooperative normals and pose composition ----
 * di2p_estimate_normals_cells (csrc/scan_prep.hip): di2p_estimate_normals with the same arguments, the same workspace and the same
 *   outputs BIT FOR BIT, computed by one workgroup per occupied grid cell (cell edge radius (1 + 2^-20)): the members of the cell's 27
 *   neighbour cells are staged in LDS once for all queries of the cell.  A cell whose candidate set has more than
 *   di2p_normals_cells_candidates() entries streams it from global memory instead; no candidate is ever dropped.
 * di2p_compose_poses (csrc/sample_prep.hip): out[b] = A[b] . Bm[b] for n row-major f64 4x4 matrices (products rounded, summed in
 *   ascending k; no FMA), one thread per frame; out may alias A or Bm. */
int di2p_normals_cells_candidates(void);
int di2p_estimate_normals_cells(const int32_t* voxel_offsets, int B, int cap, double radius, int max_nn, double max_extent, float* normals,
                                int32_t* nn_count, int32_t* nn_idx, void* workspace, void* stream);
int di2p_compose_poses(const double* A, const double* Bm, int n, double* out, void* stream);

/* ---- (additive, ABI 9; detect by symbol) evaluation mode (csrc/eval.hip): pose errors, success statistics, ENU frames ----
 * di2p_pose_errors -- evaluation/registration_lsq.py:87-95 (get_P_diff) for F frames, one thread per frame, fp64.
 *   P_pred f64[F,4,4] (its bottom row is taken as 0 0 0 1), P_gt f64[F,gt_rows,4] with gt_rows 3 or 4 (a 3-row matrix gets the row
 *   0 0 0 1, :298-299), cost f64[F] or NULL.  D = P_pred^-1 P_gt (affine inverse from the 3x3 cofactors); rte = |D[0:3,3]|; rre = the sum
 *   of the absolute extrinsic 'xzy' Euler angles of D[0:3,0:3] in degrees: with R = Ry(c) Rz(b) Rx(a), b = asin(R10), a = atan2(-R12, R11),
 *   c = atan2(-R20, R00).  enu != 0: both matrices are first multiplied on the right by the inverse of the reference's P_convert (rows
 *   1 0 0 0 / 0 0 -1 0 / 0 1 0 0 / 0 0 0 1; enu2cam, :237-248) -- the sum of |angles| is not invariant under that change of axes and the
 *   reference measures it in the converted frame.  flags i32[F]: bit 0 valid (cost > 1e-6; always set when cost is NULL), bit 1 success
 *   (rte < t_thresh and rre < r_thresh).  Within about 1e-3 deg of gimbal lock (|b| -> 90 deg) the individual angles are ill-conditioned:
 *   the result is finite there and nothing more is promised.
 * di2p_eval_accumulate -- evaluation/registration_result_analysis.py:22-47,59,63: folds one batch into the device accumulator `acc`
 *   (di2p_eval_acc_bytes() bytes, 8-byte aligned, cleared by di2p_eval_acc_reset), as 8-byte words:
 *     i64 [0] frames seen  [1] frames valid  [2] successes among the valid  [3] frames with a coarse accuracy  [4] frames with a fine accuracy
 *         [5] RTE overflow  [6] RRE overflow  [7] 0
 *     f64 [8] sum rte  [9] sum rte^2  [10] sum rre  [11] sum rre^2 (valid frames)  [12] sum coarse accuracy  [13] sum fine accuracy  [14] [15] 0
 *     i64 [16..75] RTE histogram over [0, 15) m  [76..135] RRE histogram over [0, 30) deg, 60 bins each, valid frames (np.histogram's bins;
 *         a value above the range, or NaN, goes to the overflow count)
 *   frame_mask i32[F] or NULL: a frame with mask 0 is skipped entirely (a padded last batch, a rejected raw frame).  accuracy f32[F,2]
 *   (di2p_label_accuracy's output) or NULL; a NaN accuracy (no ground-truth point inside the image) is not counted.  One workgroup; frames
 *   are added in index order, so the accumulator depends on the sequence of calls alone.
 * di2p_enu2cam_points: (x, y, z) -> (x, -z, y) for pc f32[B,3,N] (transform_pc_np(P_convert, pc) of enu2cam; exact); pc_out may be pc_in. */
long long di2p_eval_acc_bytes(void);
int di2p_pose_errors(const double* P_pred, const double* P_gt, int gt_rows, const double* cost, int enu, int F, double t_thresh,
                     double r_thresh, double* rte, double* rre, int32_t* flags, void* stream);
int di2p_eval_accumulate(const double* rte, const double* rre, const int32_t* flags, const int32_t* frame_mask, const float* accuracy, int F,
                         void* acc, void* stream);
int di2p_eval_acc_reset(void* acc, void* stream);
int di2p_enu2cam_points(const float* pc_in, float* pc_out, int B, int N, void* stream);

/* ---- (additive, ABI 9; detect by symbol) result overlays (csrc/vis.hip): the reference's per-frame images, util/vis_tools.py:96-339 ----
 * Canvas u8 [B, H + 2 H_delta, W + 2 W_delta, 3] (RGB): white, the frame's image at [H_delta : H_delta + H, W_delta : W_delta + W].  img is
 *   u8 [B,H,W,3] (img_is_u8 != 0) or f32 [B,3,H,W], converted as img.round().to(uint8): round half to even, values outside 0..255 clamped
 *   (a fork: torch leaves that conversion unspecified), NaN -> 0.
 * Points n = 0 .. N-1 in index order, later over earlier: a point is skipped if px or py is inf / NaN; cx = int(round(px)) + W_delta,
 *   cy = int(round(py)) + H_delta (half to even; tested in floating point, so 1e30 is never converted); skipped unless 0 <= cx < W_large - 1
 *   and 0 <= cy < H_large - 1.  A drawn point paints cv2.circle(radius 1, filled): (cx, cy), (cx +- 1, cy), (cx, cy +- 1), clipped.
 *   A canvas pixel therefore shows the colour of the LARGEST n whose stamp covers it: one atomicMax of ((n + 1) << 3) | colour code per stamp
 *   pixel into a u32 key plane, then one compose pass (key 0: the base pixel).  Deterministic.  N <= 2^28.  Three launches per call.
 * di2p_vis_classification -- get_classification_visualization(_coarse): pxpy f32[B,2,N] (di2p_project_labels' third output; no z test),
 *   labels i32[B,N] with values 0 / 1.  pred == 1 and gt == 1: (0,255,0), or (255,255,0) in the fine variant when fine_pred != fine_gt;
 *   gt == 1 only: (255,0,0); pred == 1 only: (0,0,255); neither: nothing is drawn and nothing is covered.  Fine variant (fine_pred, fine_gt
 *   not NULL, grid_s >= 1 the cell size): before the points, white one-pixel rows at y = h grid_s + H_delta over the image's columns for
 *   h = 1 .. n_rows and white columns at x = w grid_s + W_delta over the image's rows for w = 1 .. n_cols; the caller passes
 *   n_rows = round(H / grid_s) - 1, n_cols = round(W / grid_s) - 1 with Python's round.  Coarse variant: fine_pred == fine_gt == NULL, grid_s == 0.
 * di2p_vis_registration -- get_registration_visualization: pc f32[B,3,N] widened to f64, P f64[B,4,4], K f64[B,3,3]; q = rows 0..2 of
 *   P [p; 1], k = K q (products rounded, summed left to right, no FMA), px = k0 / k2, py = k1 / k2; additionally skipped when k2 < 0.
 *   labels i32[B,N]: (255,0,0) where 1, else (0,0,255).
 * workspace: di2p_vis_workspace_bytes() bytes (the key plane, rounded up to 256; -1 for bad sizes), 16-byte aligned, cleared by every call.
 * cv2.putText (t_ij_np) is not reproduced. */
long long di2p_vis_workspace_bytes(int B, int H, int W, int H_delta, int W_delta);
int di2p_vis_classification(const float* pxpy, const int32_t* coarse_pred, const int32_t* coarse_gt, const int32_t* fine_pred,
                            const int32_t* fine_gt, const void* img, int img_is_u8, int B, int N, int H, int W, int H_delta, int W_delta,
                            int grid_s, int n_rows, int n_cols, uint8_t* canvas, void* workspace, void* stream);
int di2p_vis_registration(const float* pc, const double* P, const double* K, const int32_t* labels, const void* img, int img_is_u8, int B, int N,
                          int H, int W, int H_delta, int W_delta, uint8_t* canvas, void* workspace, void* stream);

/* ---- (additive, ABI 9; detect by symbol) Oxford sub-map building from LMS push-broom profiles (csrc/submap.hip) -----------------------------
 * Replaces data/oxford/build_dataset.py:79-148 (my_build_pointcloud) and :310,319-321 (camera frame, float32 record); the voxel pass between
 * them (:151-166) is di2p_voxel_down_sample at 0.1 m on the float32 rows di2p_submap_build writes.
 * A batch of B sub-maps of one traversal, ragged on two levels (all device memory): scan_xyr f64[P_cap,3] the rows of the .bin files (x, y,
 *   reflectance; x points to the ground), scan_offsets i32[S_cap+1] profile -> rows, submap_offsets i32[B+1] sub-map -> profiles, poses
 *   f64[S_cap,4,4] the pose of each profile relative to its sub-map's origin time (rigid), present u8[S_cap] (may be NULL: all present; 0: the
 *   scan file does not exist), G_posesource_laser f64[4,4].  S_cap / P_cap: the capacities of the profile / row buffers; entries past
 *   submap_offsets[B] / the last scan offset are never read.
 * di2p_submap_build, six launches, no allocation, no synchronisation:
 *   keep rule, sequential per sub-map: a missing profile is passed over; a present one is skipped iff skip_threshold >= 0, a previous KEPT
 *     profile exists and |R_prev^T (t - t_prev)|^2 < skip_threshold^2 in fp64 (products rounded, sums in ascending index; the translation of
 *     inv(prev) . pose with the squares compared).  kept i32[S_cap]: 1 kept, 0 skipped, -1 missing or outside every accepted sub-map;
 *     skip_count i32[B].  A kept profile is the next "previous" even if the ground filter leaves it no rows.
 *   rows: with remove_ground != 0 a row survives iff x < ground_threshold (fp64).  M = pose . G_posesource_laser per kept profile, each entry
 *     a dot product in ascending k; p = (M[:,0] x + M[:,1] y) + M[:,3], no fused multiply-add; out_points f32[cap,4] rows (p_x, p_y, p_z,
 *     reflectance), each value rounded once, in profile order, then row order (stable); out_offsets i32[B+1].
 *   status i32[B] (may be NULL): 0 ok; 1 more than max_frame_points (<= 2^20) surviving rows, or rows that would pass cap; 3 bad offsets
 *     (submap_offsets[0 .. b+1] not a non-decreasing sequence in [0, S_cap] from 0, or a profile of the sub-map without
 *     0 <= scan_offsets[s] <= scan_offsets[s+1] <= P_cap); 4 no profile or no surviving row.  A sub-map with a status has no output rows.
 *   workspace: di2p_submap_workspace_bytes(B, S_cap) bytes, 256-byte aligned.
 * di2p_scan_prep_centroids_offset (csrc/scan_prep.hip): byte offset, in the workspace di2p_voxel_down_sample ran with (same B, cap), of
 *   its fp64 means f64[cap,3] in output point order (-1 for bad sizes); valid until the next call that uses the workspace.
 * di2p_submap_to_camera: row v of sub-map b (voxel_offsets i32[B+1]) -> out_points f32[cap,4] = (G_cam[b] . (centroids[v], 1) in fp64,
 *   ascending k, no fused multiply-add, rounded once; intensity[v]).  G_cam f64[B,4,4] = inv(G_camera_image) . G_camera_posesource. */
long long di2p_submap_workspace_bytes(int B, int S_cap);
int di2p_submap_build(const double* scan_xyr, const int32_t* scan_offsets, const int32_t* submap_offsets, const double* poses,
                      const uint8_t* present, const double* G_posesource_laser, int B, int S_cap, int P_cap, int cap, int max_frame_points,
                      double skip_threshold, double ground_threshold, int remove_ground, int32_t* kept, int32_t* skip_count,
                      int32_t* out_offsets, float* out_points, int32_t* status, void* workspace, void* stream);
long long di2p_scan_prep_centroids_offset(int B, int cap);
int di2p_submap_to_camera(const double* centroids, const float* intensity, const int32_t* voxel_offsets, const double* G_cam, int B, int cap,
                          float* out_points, void* stream);

/* ---- (additive, ABI 9; detect by symbol) nuScenes sweep accumulation (csrc/sweeps.hip) -------------------------------------------------------
 * Replaces the raw stage of data/nuscenes_pc_img_pose_loader.py: :58-78 (pose and calibration matrices), :194-210 (the ego-box filter of a
 * sweep), :213-267 (the accumulation of up to seven sweeps in the key sweep's LiDAR frame) and :292-293, :324-325, :351-354 (P_cam_pc).
 * di2p_pose_matrices: records f64[n,7] (quaternion w, x, y, z, translation) -> out f64[n,4,4]: q / |q|, the closed form of the rotation
 *   matrix in fp64 (products and sums rounded separately), every rotation entry and the translation rounded to float32; last row 0 0 0 1.
 * A batch of B frames, ragged on two levels (all device memory): rows f32[P_cap,cols], cols 4 (x, y, z, intensity) or 5 (the .pcd.bin rows;
 *   the ring is not read), sweep_offsets i32[S_cap+1] sweep -> rows, frame_offsets i32[B+1] frame -> sweeps, the key sweep first, then the
 *   `next` picks, then the `prev` picks.  Entries past frame_offsets[B] / the last sweep offset are never read.
 * di2p_sweep_transforms: P_ego f64[S_cap,4,4] the ego pose of every sweep, P_vehicle_lidar / P_ego_cam / P_vehicle_cam f64[B,4,4] the LiDAR
 *   calibration, the camera's ego pose and the camera calibration of every frame (affine: the last row is taken as 0 0 0 1) ->
 *   T f64[S_cap,4,4]: the exact identity for a frame's first sweep, else (inv(P_vehicle_lidar) . (inv(P_ego[key]) . P_ego[s])) . P_vehicle_lidar;
 *   P_cam_pc f64[B,4,4] = inv(P_vehicle_cam) . (inv(P_ego_cam) . (P_ego[key] . P_vehicle_lidar)) (zeros for a frame without a sweep).  fp64,
 *   4x4 products in ascending k, inverses as adj(M) / det(M) and -(M^-1 . t); no fused multiply-add.  A frame whose sweep range does not lie
 *   in [0, S_cap] is left alone.
 * di2p_sweep_accumulate, six launches, no allocation, no synchronisation: a row is removed iff -box_x < x < box_x and -box_y < y < box_y
 *   in float32; the surviving rows of a frame in sweep order, then row order (stable) -> out_points f32[cap,4]: rows of the key sweep and every
 *   intensity bit for bit, the coordinates of the other sweeps ((T[r,0] x + T[r,1] y) + T[r,2] z) + T[r,3] in fp64, rounded once to float32;
 *   out_offsets i32[B+1]; kept i32[S_cap] surviving rows per sweep (0 outside the accepted frames).  Rows past out_offsets[B] are not written.
 *   status i32[B] (may be NULL): 0 ok; 1 more than max_frame_points (<= 2^20) surviving rows, or rows that would pass cap; 3 bad offsets
 *     (frame_offsets[0 .. b+1] not a non-decreasing sequence in [0, S_cap] from 0, or a sweep of the frame without
 *     0 <= sweep_offsets[s] <= sweep_offsets[s+1] <= P_cap); 4 no sweep or no surviving row.  A frame with a status has no output rows.
 *   workspace: di2p_sweep_workspace_bytes(B, S_cap) bytes (0 for bad sizes; S_cap <= 2^24), 256-byte aligned. */
long long di2p_sweep_workspace_bytes(int B, int S_cap);
int di2p_pose_matrices(const double* records, int n, double* out, void* stream);
int di2p_sweep_transforms(const double* P_ego, const int32_t* frame_offsets, const double* P_vehicle_lidar, const double* P_ego_cam,
                          const double* P_vehicle_cam, int B, int S_cap, double* T, double* P_cam_pc, void* stream);
int di2p_sweep_accumulate(const float* rows, const int32_t* sweep_offsets, const int32_t* frame_offsets, const double* T, int B, int S_cap,
                          int P_cap, int cols, int cap, int max_frame_points, float box_x, float box_y, int32_t* kept, int32_t* out_offsets,
                          float* out_points, int32_t* status, void* workspace, void* stream);

/* ---- (additive, ABI 9; detect by symbol) synthetic worlds (csrc/world.hip) ---------------------------------------------------------------------
 * One analytic scene per frame, ray-cast for the camera and for an HDL-64-like LiDAR through one trace function (deepi2p_amd/world.py fixes
 * the formulas; tests/world_oracle.py restates them in numpy).  prims f64[B,P,16], P <= 32 (checked), count i32[B] (clamped to [0, P] on the
 * device; 0: all sky, no return).  A row: type (0 ground, 1 box, 2 vertical cylinder); ground z0 | box lo xyz, hi xyz | cylinder cx, cy,
 * radius, z0, z1 in slots 1-6; albedo r g b in [0, 1] (7-9); LiDAR reflectance (10); texture cell size > 0 (11); 12-15 unused.
 * di2p_world_trace: origin f64[B,3], dirs f64[B,R,3] -> t f64[B,R] (inf on a miss), prim i32[B,R] (-1 on a miss): the nearest hit, ties to
 *   the lowest index; fp64, no fused multiply-add; slab test with 1 / d (NaN products skipped), smaller cylinder root, ground for d.z < 0.
 * di2p_world_render_camera: pixel (u, v) casts cam_to_world[b] . ((u - cx) / fx, (v - cy) / fy, 1) from cam_to_world[b]'s translation
 *   (K_raw f64[B,3,3], cam_to_world f64[B,4,4] used as given) -> image u8[B,H0,W0,3] (4-byte aligned; dword stores, correct for any H0, W0),
 *   and where not NULL depth f32[B,H0,W0] (t, 0 on a miss) and prim i32[B,H0,W0].  max_range: the distance at which the fade ends.
 * di2p_world_render_scan, four launches, no allocation, no synchronisation: ray r = beam * azimuths + azimuth has the sensor-frame direction
 *   (cE cA, cE sA, sE) from elevation f64[beams,2] and azimuth f64[B,azimuths,2] (cos, sin), cast from pose f64[B,4,4] (sensor to world).  Kept
 *   iff t < max_range and u >= dropout (before the noise); t += range_sigma g, intensity = clip(reflectance + intensity_sigma g', 0, 1); u, g,
 *   g' from Philox counter (r, frame0 + b, 0 | 1 | 2, 7), seed = *seed_dev if seed_dev else seed.  -> out_points f32[B * beams * azimuths, 4]
 *   rows (x, y, z, intensity) in the sensor frame, the kept rays in ray order, frame after frame; out_offsets i32[B+1]; out_count i32[B].
 *   Rows past out_offsets[B] are not written.  workspace: di2p_world_workspace_bytes(B, beams * azimuths) bytes (0 for bad sizes), 256-byte
 *   aligned.  B <= 65535 and B * R < 2^31 everywhere. */
long long di2p_world_workspace_bytes(int B, int R);
int di2p_world_trace(const double* prims, const int32_t* count, int B, int P, const double* origin, const double* dirs, int R, double* t,
                     int32_t* prim, void* stream);
int di2p_world_render_camera(const double* prims, const int32_t* count, int B, int P, const double* K_raw, const double* cam_to_world, int H0,
                             int W0, double max_range, uint8_t* image, float* depth, int32_t* prim, void* stream);
int di2p_world_render_scan(const double* prims, const int32_t* count, int B, int P, const double* elevation, const double* azimuth,
                           const double* pose, int beams, int azimuths, double max_range, double dropout, double range_sigma,
                           double intensity_sigma, unsigned long long seed, const unsigned long long* seed_dev, int frame0, float* out_points,
                           int32_t* out_offsets, int32_t* out_count, void* workspace, void* stream);

/* ---- (additive, ABI 9; detect by symbol) push-broom profiles of a synthetic world (csrc/world.hip) ----------------------------------------------
 * di2p_world_render_profiles, six launches, no allocation, no synchronisation: a 2-D laser carried through one scene per SUB-MAP (prims
 *   f64[B,P,16], count i32[B] as above), with one pose per PROFILE.  Profiles of sub-map b: [submap_offsets[b], submap_offsets[b+1]) (i32[B+1]).
 *   Beam k of profile s casts R_s . (c_k, s_k, 0) from the translation of laser_to_world[s] (f64[S_cap,4,4], used as given; beam f64[beams,2]
 *   holds (cos, sin) of the angle in the laser's x-y plane; every entry of the direction is a sum of three rounded products in ascending index,
 *   the last one with 0).  Kept iff t < max_range and u >= dropout (before the noise); t += range_sigma g; the row is (t c_k, t s_k,
 *   clip(255 (reflectance + reflectance_sigma g'), 0, 255)) in float64, not rounded to an integer.  u, g, g' from Philox counter
 *   (k, frame0 + s, 0 | 1 | 2, 8), seed = *seed_dev if seed_dev else seed.
 *   -> scan_xyr f64[S_cap * beams, 3] (the kept rays in beam order, profile after profile; rows past scan_offsets[S_cap] are not written),
 *   scan_offsets i32[S_cap+1] (entries past submap_offsets[B] hold the end of the rows), out_count i32[S_cap]: the first two arguments of
 *   di2p_submap_build.  status i32[B]: 0, or 3 for a sub-map whose offsets submap_offsets[0 .. b+1] are not a non-decreasing sequence in
 *   [0, S_cap] that starts at 0 (that sub-map and every later one have no rows; nothing is read out of range).
 *   workspace: di2p_world_profiles_workspace_bytes(S_cap, beams) bytes (0 for bad sizes), 256-byte aligned.  B <= 65535, S_cap * beams < 2^31. */
long long di2p_world_profiles_workspace_bytes(int S_cap, int beams);
int di2p_world_render_profiles(const double* prims, const int32_t* count, int B, int P, const int32_t* submap_offsets, const double* laser_to_world,
                               const double* beam, int S_cap, int beams, double max_range, double dropout, double range_sigma,
                               double reflectance_sigma, unsigned long long seed, const unsigned long long* seed_dev, int frame0, double* scan_xyr,
                               int32_t* scan_offsets, int32_t* out_count, int32_t* status, void* workspace, void* stream);

/* ---- (additive, ABI 9; detect by symbol) pose confidence (csrc/solver_aux.hip): information matrix, covariance, restart consensus ----------------------
 * No allocation, no synchronisation, no atomics: every entry point can be captured into a hipGraph, and a frame's outputs are bit-identical
 * from run to run and do not depend on F or on the frame's position in the batch.
 * WHAT THE NUMBERS ARE.  info, grad and cov live in the SOLVER's parameterisation ([ry, tx, ty, tz] or [angle-axis, t] of the points the
 *   solve was given; for a frame="enu" pipeline that is the pose P_cam of the converted points, not P).  No noise scale is fitted: the
 *   residuals are pixels (and 100 x metres behind the camera) under a Cauchy loss of scale 1, so cov = info^-1 is NOT a covariance in
 *   metres^2 / radians^2 of the expected pose error.  sigma_t and sigma_r are a RELATIVE measure between frames of one configuration (same
 *   camera, image size, point count, labels source): a larger value means a flatter minimum, nothing more.
 * di2p_pose_information: at given parameters, the Cauchy-weighted normal matrix the Levenberg-Marquardt step uses (and Ceres' covariance
 *   would): info f64[F,np,np] = sum over residual blocks of rho'(s) J^T J (full symmetric matrix, rho' = 1 / (1 + s), s = |r_block|^2; a
 *   label-1 point is a block of 3 rows, a label-0 point a block of 1, residuals and Jacobians those of registration_2d.hpp /
 *   registration_3d.hpp, the angle-axis rotation with its first-order branch at theta^2 <= DBL_EPSILON), grad f64[F,np] = sum rho'(s) J^T r
 *   (the gradient of the cost), cost f64[F] = 1/2 sum log1p(s), active i32[F,2] = the label-1 and the label-0 points with a non-zero
 *   residual block (the points that constrain the pose).  points f32[F,3,N] (widened per element), labels i32[F,N] (anything outside
 *   {0, 1} is skipped: di2p_initial_guess' labels_out works as it is), K f64[F,3,3], params f64[F,np], np = 4 if is_2d else 6.
 *   Two launches: grid (F, C), C = ceil(N / 1024), every workgroup reducing its 1024 points in a fixed order into the workspace, then the C
 *   partials of a frame added in index order.  workspace: di2p_pose_information_workspace_bytes(F, N) bytes, 8-byte aligned.  N <= 65535 * 1024.
 * di2p_gather_best_params: out f64[F,np] = params[f, best[f]] of params f64[F,R,np] (di2p_select_best's best; a frame with best outside
 *   [0, R) -- has_inside == 0 -- takes restart 0).
 * di2p_pose_covariance: cov f64[F,np,np] = the inverse of info over the FREE parameters, by fp64 Cholesky, one thread per frame.  A
 *   translation parameter exactly on its bound (x == lb or x == ub; the solver projects onto the box, so equality is exact) is fixed: its
 *   row and column are removed before the inversion and its entries of cov are 0.  free_mask i32[F]: bit i set = parameter i is free.
 *   status i32[F]: 0 ok; 1 not positive definite (a pivot <= np * DBL_EPSILON * max_i info_ii over the free i, or no free parameter);
 *   2 has_inside[f] == 0 (has_inside may be NULL) or a non-finite entry of info or params.  sigma_t f64[F] = sqrt(trace of the translation
 *   block of cov), sigma_r f64[F] = sqrt(trace of the rotation block) * 180 / pi.  For status != 0 cov, sigma_t and sigma_r are NaN;
 *   free_mask is written all the same.  cov is exactly symmetric.  lb_host / ub_host: f64[3] HOST arrays, the solve's bounds.
 * di2p_restart_consensus: params f64[F,R,np], cost f64[F,R] (di2p_solve_batched's outputs), best i32[F] -> finite i32[F]: restarts with a
 *   finite cost; agree i32[F]: those of them whose pose is within t_tol and r_tol_deg of the best one's, by get_P_diff's rule (the device
 *   code of di2p_pose_errors) on P_r^-1 P_best: translation norm < t_tol and summed absolute 'xzy' Euler angles in degrees < r_tol_deg; the
 *   best counts itself.  gap f64[F] = (smallest cost among the finite restarts that do not agree) - cost[best]; +inf when all agree.  A frame
 *   with has_inside[f] == 0 (may be NULL) or best outside [0, R) gets finite = agree = 0 and gap = NaN.  One wave per frame, any R >= 1. */
long long di2p_pose_information_workspace_bytes(int F, int N);
int di2p_pose_information(const float* points, const int32_t* labels, const double* K, const double* params, double H, double W, int is_2d,
                          int F, int N, double* info, double* grad, double* cost, int32_t* active, void* workspace, void* stream);
int di2p_gather_best_params(const double* params, const int32_t* best, int is_2d, int F, int R, double* out, void* stream);
int di2p_pose_covariance(const double* info, const double* params, const int32_t* has_inside, const double* lb_host, const double* ub_host,
                         int is_2d, int F, double* cov, int32_t* free_mask, int32_t* status, double* sigma_t, double* sigma_r, void* stream);
int di2p_restart_consensus(const double* params, const double* cost, const int32_t* best, const int32_t* has_inside, int is_2d, int F, int R,
                           double t_tol, double r_tol_deg, int32_t* finite, int32_t* agree, double* gap, void* stream);

/* ---- (additive, ABI 9; detect by symbol) map localisation (csrc/map_index.hip): cell index, prior crops, camera pose in the map -------------------
 * The map is points f32[M,4] rows (x, y, z, intensity) in a map frame; the caller keeps its coordinates small enough for float32 (relative to
 *   a map origin of its own).  up_axis in {0, 1, 2} names the vertical axis, the ground axes (a, b) are the other two in ascending order
 *   (camera-convention maps, y down: up_axis 1, ground plane x-z; z-up maps: up_axis 2).  The grid: origin (origin0, origin1) on (a, b), cell
 *   metres (> 0), nx x ny cells, nx ny <= 2^24; M <= 2^27.  All index arithmetic is fp64, every operation rounded once, no fused multiply-add.
 * di2p_map_index_build, eager, once per map; refuses (returns -1, nothing enqueued, the capture stays usable) while `stream` is capturing.
 *   Cell of a row: ix = floor(((double)p[a] - origin0) / cell), iy likewise on b, id = iy nx + ix.  -> cell_start i32[nx ny + 1]; order i32[M]
 *   the map row of every stored row; sorted f32[M,4] the rows cell after cell in ascending id, inside a cell in ascending map row (a stable
 *   sort); status i32[1]: 0, or 1 when a coordinate is not finite or a row falls outside the grid (the arrays are then unspecified).
 *   workspace: di2p_map_index_workspace_bytes(M, nx ny) bytes (0 for bad sizes), 256-byte aligned.
 * di2p_map_crop, five launches, no allocation, no synchronisation, no memset node, no atomics: T_map_prior f64[B,4,4] (map <- prior frame),
 *   radius f64[B] (both device memory, read inside the launches).  Frame b: centre c = (T[a][3], T[b][3]); window
 *   ix0 = max(0, floor(((c0 - r) - origin0) / cell)), ix1 = min(nx - 1, floor(((c0 + r) - origin0) / cell)), iy0 and iy1 likewise; window
 *   cells are visited iy-major (iy ascending outside, ix ascending inside), the rows of a cell in stored order.  A row is kept iff
 *   dx dx + dy dy < r r (strict) with dx = (double)p[a] - c0, dy = (double)p[b] - c1, and written in the prior frame: with
 *   d_k = (double)p[k] - T[k][3], q_i = (float)((T[0][i] d0 + T[1][i] d1) + T[2][i] d2); the intensity bit for bit.
 *   -> rows f32[cap,4], offsets i32[B+1], index i32[cap] (may be NULL) the map row of every kept row.  Rows past offsets[B] are not written.
 *   status i32[B] (may be NULL): 0 ok; 1 more than max_frame_points (<= 2^20) kept rows, rows that would pass cap, or a window of more than
 *     max_cells cells; 4 no kept row (also a disc that misses the grid); 5 a non-finite entry of the prior, or a radius that is not finite and
 *     positive.  A frame with a status has no rows (offsets[b+1] = offsets[b]) and leaves every other frame's rows as they are without it.
 *   workspace: di2p_map_crop_workspace_bytes(B, max_cells) bytes (0 for bad sizes; B max_cells <= 2^28), 256-byte aligned.
 * di2p_map_pose: T_map_cam[b] = T_map_prior[b] . P_scan[b]^-1 for n row-major f64 4x4 matrices, the inverse as the rigid [R^T | -R^T t]
 *   (P_scan's last row is not read), the product as di2p_compose_poses writes it; T_map_cam may be one of the inputs. */
long long di2p_map_index_workspace_bytes(int M, int ncell);
long long di2p_map_crop_workspace_bytes(int B, int max_cells);
int di2p_map_index_build(const float* points, int M, int up_axis, double origin0, double origin1, double cell, int nx, int ny,
                         int32_t* cell_start, int32_t* order, float* sorted, int32_t* status, void* workspace, void* stream);
int di2p_map_crop(const float* sorted, const int32_t* cell_start, const int32_t* order, int M, int up_axis, double origin0, double origin1,
                  double cell, int nx, int ny, const double* T_map_prior, const double* radius, int B, int cap, int max_frame_points,
                  int max_cells, float* rows, int32_t* offsets, int32_t* index, int32_t* status, void* workspace, void* stream);
int di2p_map_pose(const double* T_map_prior, const double* P_scan, int n, double* T_map_cam, void* stream);

/* ---- (additive, ABI 9; detect by symbol) normals of a map and crops that carry them (csrc/map_normals.hip, csrc/map_index.hip): the KITTI model ----
 * di2p_map_normals, eager, once per map; refuses (returns -1, nothing enqueued, the capture stays usable) while `stream` is capturing.
 *   di2p_estimate_normals' definition with the map as one frame and the row itself as the point: points f32[M,4], 1 <= M <= 2^27, radius
 *   finite and > 0, 1 <= max_nn <= 64, up_axis in {0, 1, 2}, orient +1 or -1 (-1 for camera-convention maps, where up is -y).
 *   Neighbours of row q: the at most max_nn rows j with d2 < radius^2, q included, d2 = ((dx dx + dy dy) + dz dz) in fp64 on (double) of the
 *   float32 coordinates, taken in ascending (d2, j), j the row number in `points`; exact whatever the density; duplicated rows are distinct
 *   neighbours.  Normal: the eigenvector of the smallest eigenvalue of the neighbours' covariance (butterfly sums, cyclic Jacobi, fp64);
 *   orient . e_up_axis for fewer than 3 neighbours or a zero covariance; otherwise flipped so that orient . n[up_axis] >= 0.  With
 *   up_axis 2, orient +1 the outputs are di2p_estimate_normals' bit for bit on the same points (one implementation: csrc/normals_nn.h).
 *   The grid: cell edge radius (1 + 2^-20) over the map's own bounds, 21 bits per axis in a 63-bit key, a stable radix sort of (key, row).
 *   -> normals f32[M,3], nn_count i32[M] (may be NULL), nn_idx i32[M,max_nn] (may be NULL; -1 past the count), all in the order of the rows
 *   given; status i32[1]: 0; 1 a non-finite coordinate; 2 a bounds edge above radius (2^21 - 4).  With a status nothing else is written.
 *   workspace: di2p_map_normals_workspace_bytes(M) bytes (0 for a bad size; about 64 M), 256-byte aligned; points 16-byte aligned.
 * di2p_map_crop_normals, one launch behind di2p_map_crop, no allocation, no synchronisation, no memset node, no atomics; offsets (the crop's)
 *   and T_map_prior are read from device memory inside the launch.  For every kept row k < offsets[B] of frame b, with
 *   n = (double)normals[index[k]] (normals f32[M,3] in map-row order, index the crop's):
 *   out[k][i] = (float)((T[0][i] n0 + T[1][i] n1) + T[2][i] n2), R^T n, every operation rounded once.  Rows past offsets[B] are not written. */
long long di2p_map_normals_workspace_bytes(int M);
int di2p_map_normals(const float* points, int M, int up_axis, int orient, double radius, int max_nn, float* normals, int32_t* nn_count,
                     int32_t* nn_idx, int32_t* status, void* workspace, void* stream);
int di2p_map_crop_normals(const float* normals, const int32_t* index, const int32_t* offsets, const double* T_map_prior, int B, int cap, float* out,
                          void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DEEPI2P_HIP_H */
