// Host entry points of the gfx950 kernels: every rk:: function a binding
// translation unit calls, declared once. Each .hip file includes this header,
// so a definition is checked against its declaration, and default arguments
// are stated here and nowhere else.

#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace rk {
void mfma_probe(const float* a, const float* b, float* d, hipStream_t stream);
void embed_mlp_fwd(const uint8_t* ids, const void* w1, const float* b1,
                   const void* w2, const float* b2, const void* emb, void* out,
                   int B, hipStream_t stream, uint32_t dbg,
                   unsigned long long* timing);
void embed_mlp_fwd2(const uint8_t* ids, const void* w1g, const float* b1,
                    const void* w2, const float* b2, const void* emb,
                    void* out, int B, hipStream_t stream);
void embed_mlp_fwd3(const uint8_t* ids, const void* w1g, const float* b1,
                    const void* w2, const float* b2, const void* emb,
                    void* out, int B, hipStream_t stream,
                    unsigned long long* timing, int ldo = 500);
void embed_mlp_fwd4(const uint8_t* ids, const void* w1g, const float* b1,
                    const void* w2, const float* b2, const void* emb,
                    void* out, int B, hipStream_t stream,
                    unsigned long long* timing, int ldo = 500,
                    int max_blocks = 0);
void gru_layer_fwd(const void* xg, const void* u, const float* bhh, void* hseq,
                   void* cache, int T, int B, hipStream_t stream, uint32_t dbg,
                   int impl = 0);
int gru_eval_select(int impl, int B);
void gru_layer_fwd_fused(const void* x, const void* w_ih_p, const void* b_ih,
                         const void* u, const float* bhh, void* xg_ws,
                         void* hseq, int T, int B, int IN, int KP,
                         hipStream_t stream);
void gru_layer_bwd(const void* cache, const void* hseq, const void* dhin,
                   const void* ut, void* dxg, void* dhg, int T, int B,
                   hipStream_t stream, uint32_t dbg);
void ce_fwd_bwd(const float* logits, const int64_t* target, float* dlogits,
                float* loss_sum, int64_t n, hipStream_t stream);
void adam_step(float* p, const float* g, float* m, float* v, int64_t n,
               float lr, float beta1, float beta2, float eps, int step,
               hipStream_t stream, const int* step_ptr);
void adam_mt(const int64_t* table, int n_params, float* p, float* m, float* v,
             float lr, float beta1, float beta2, float eps, int step,
             hipStream_t stream, const int* step_ptr);
void grad_gather(const int64_t* table, int n_params, float* flat_g,
                 hipStream_t stream);
void head_fwd(const void* hseq, const void* w4, const float* b4, float* logits,
              uint8_t* amax, int T, int B, hipStream_t stream,
              uint8_t* qv = nullptr);
void emb_grad(const void* dm, const uint8_t* ids, float* de, int64_t n,
              hipStream_t stream);
void front_fwd(const uint8_t* ids, const void* w1, const float* b1,
               const void* w2, const float* b2, const void* emb, void* out,
               int B, uint32_t seed, float keep, hipStream_t stream,
               const uint32_t* seed_ptr);
void front_bwd(const uint8_t* ids, const void* dseq, const void* w1,
               const float* b1, const void* w2, const float* b2,
               const void* emb, float* dw1, float* db1, float* dw2, float* db2,
               const void* w1t_g, float* de, int B, uint32_t seed, float keep,
               hipStream_t stream, uint32_t phase_mask,
               const uint32_t* seed_ptr, const void* w1g);
void gemm_bias(const void* A, const void* B, const float* bias, void* C,
               int M, int N, int K, hipStream_t stream);
void xg_gemm2(const void* A, const void* Bt, const void* bias, void* C,
              int M, int KREAL, int KP, hipStream_t stream,
              unsigned long long* timing = nullptr);
void xg_gemm3(const void* A, int lda, const void* Bt, const void* bias,
              void* C, int M, int KP, hipStream_t stream);
int xg_gemm3_tile_m();
void xg_gemm3_stamped(const void* A, int lda, const void* Bt,
                      const void* bias, void* C, int M, int KP,
                      unsigned long long* stamps, hipStream_t stream);
int xg_gemm3_stamp_words();
void xg_gemm4(const void* A, int lda, const void* Bt, const void* bias,
              void* C, int M, int KP, int max_wgs, hipStream_t stream);
void xg_gemm4w(const void* A, int lda, const void* Bt, const void* bias,
               void* C, int M, int max_wgs, hipStream_t stream);
int xg_gemm4w_tile_m();
bool xg_gemm4w_pays(int M);
int xg_gemm4_cus();
int atb_splitk_nslices(int K);
void atb_splitk(const void* A, const void* B, float* ws, float* C, int M,
                int N, int K, hipStream_t stream);
void atb_splitk_ld(const void* A, int lda, const void* B, int ldb,
                   float* ws, float* C, int M, int N, int K,
                   hipStream_t stream);
void colsum_f32(const void* X, int ldx, int K, int N, float* out,
                float* part, hipStream_t stream);
void front_de(const uint8_t* ids, const void* dt1g, const void* w1t_g,
              float* de, int B, uint32_t seed, float keep, hipStream_t stream,
              unsigned long long* timing, uint32_t dbg,
              const uint32_t* seed_ptr);
void vote_scatter(const uint8_t* preds, const int32_t* positions,
                  uint32_t* table, int64_t n_slots, uint32_t* err_flag,
                  int n_cols, hipStream_t stream);
void vote_consensus(const uint32_t* table, int64_t n_slots, uint8_t* maj,
                    hipStream_t stream);
void vote_scatter_q(const uint8_t* preds, const uint8_t* units,
                    const int32_t* positions, uint32_t* table, uint64_t* qsum,
                    int64_t n_slots, uint32_t* err_flag, int n_cols,
                    hipStream_t stream);
void vote_consensus_q(const uint32_t* table, const uint64_t* qsum,
                      int64_t n_slots, uint8_t* maj, uint8_t* qual,
                      hipStream_t stream);
int64_t edit_num_blocks(int64_t n_pos);
void edit_bounds(const uint32_t* table, int64_t n_pos, int64_t* state,
                 hipStream_t stream);
void edit_scan(int64_t* counts, int64_t n, int64_t* state,
               hipStream_t stream);
void edit_count(const uint32_t* table, const uint8_t* draft, int64_t n_pos,
                int64_t* state, int64_t* counts, hipStream_t stream);
void edit_write(const uint32_t* table, const uint64_t* qsum,
                const uint8_t* draft, int64_t n_pos, const int64_t* state,
                const int64_t* offsets, void* records, int64_t total,
                hipStream_t stream);
void stitch_count(const uint32_t* table, const uint64_t* qsum,
                  const uint8_t* draft, int64_t n_pos, int64_t* state,
                  int64_t* counts, int min_qual, bool keep_uncovered,
                  hipStream_t stream);
void stitch_write(const uint32_t* table, const uint64_t* qsum,
                  const uint8_t* draft, int64_t n_pos, const int64_t* state,
                  const int64_t* offsets, int min_qual, bool keep_uncovered,
                  uint8_t* seq, uint8_t* qual, int64_t total,
                  hipStream_t stream);
bool windows_geometry_ok(int rows, int cols, int stride, int max_ins);
void windows_index(const int32_t* ref_start, const int32_t* ref_end,
                   const uint8_t* reverse, const uint32_t* cigar_off,
                   const uint32_t* seq_off, const uint32_t* cigar,
                   const uint8_t* seq4, int32_t* op_rpos, int32_t* op_qpos,
                   int n, int start, int end, int32_t* diff, int32_t* insd,
                   int32_t* col0, int32_t* colpos, int ncols_max,
                   int n_all_max, unsigned long long* mask, int32_t* wpre,
                   int32_t* nvalid, int32_t* out_idx, int32_t* meta,
                   hipStream_t stream);
void windows_fill(const int32_t* ref_start, const int32_t* ref_end,
                  const uint8_t* reverse, const uint32_t* cigar_off,
                  const uint32_t* seq_off, const uint32_t* cigar,
                  const uint8_t* seq4, int32_t* op_rpos, int32_t* op_qpos,
                  int n, int start, int end, const int32_t* col0,
                  const int32_t* colpos, const unsigned long long* mask,
                  const int32_t* wpre, const int32_t* nvalid,
                  const int32_t* out_idx, uint64_t region_key, int n_all,
                  int n_out, uint8_t* x, int32_t* pos, hipStream_t stream);
void truth_scan(const int32_t* ref_start, const int32_t* ref_end,
                const uint32_t* cigar_off, const uint32_t* seq_off,
                const uint32_t* cigar, const uint8_t* seq4, int32_t* op_rpos,
                int32_t* op_qpos, int n, int32_t* err, hipStream_t stream);
void label_windows(const int32_t* ref_start, const int32_t* ref_end,
                   const uint32_t* cigar_off, const uint32_t* seq_off,
                   const uint32_t* cigar, const uint8_t* seq4,
                   int32_t* op_rpos, int32_t* op_qpos, int n, int index,
                   int lo, int hi, const int32_t* pos, int n_windows,
                   uint8_t* labels, uint8_t* keep, int32_t* err,
                   hipStream_t stream);
void gather_batch(const uint8_t* X, const uint8_t* Y, const int32_t* idx,
                  uint8_t* out_x, int64_t* out_y, int64_t B,
                  hipStream_t stream);
void eval_metrics(const float* logits, const uint8_t* labels, int64_t n,
                  double inv_n, uint64_t* correct, double* loss_sum,
                  hipStream_t stream);
int wfa_probe();
int wfa_coop();
int wfa_pad();
int64_t wfa_dir_cells(int64_t n, int64_t m, int64_t s0, int64_t s1);
void wfa_steps(const uint8_t* q, const uint8_t* t, int n, int m, int s0,
               int s1, int* offs, uint8_t* dir, int* done, hipStream_t stream);
void wfa_trace(const uint8_t* dir, int n, int m, int s0, int s_hi, int* walk,
               uint8_t* ops, hipStream_t stream);
}  // namespace rk
