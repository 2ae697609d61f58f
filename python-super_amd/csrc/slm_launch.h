// slm_launch.h -- the launch functions of the LM solver's kernels, declared once, with their default arguments:
// the LM host (slm_api.hip, slm_bind.hip, slm_lm.hip, slm_terms.hip) calls them; the file that holds the kernels defines them and includes this too, so its definitions are
// compiled against these declarations (a drifted return type or a repeated default argument does not compile; a
// drifted parameter list is still only caught when the library is loaded).
#pragma once
#include "slm_common.h"

// slm_data.hip
// (wa: the weighted variant of an enabled solver, slm_enable_data_weights; null: the kernels as they always were)
struct DataWArgs;
void launch_data_grad(const FrameDev*, int, int, int, double, hipStream_t, const DataWArgs* wa = nullptr);
void launch_data_grad_pairs(const FrameDev*, int, int, int, double, hipStream_t, const DataWArgs* wa = nullptr);
void launch_data_loss(const FrameDev*, int, int, int, double, int, hipStream_t, const DataWArgs* wa = nullptr);
void launch_data_weights(const FrameDev*, int slot, int N, int K, double lam, const DataWArgs& wa, double* w, hipStream_t);
void launch_data_resid(const FrameDev*, int, int, int, double, double*, uint8_t*, int32_t*, hipStream_t);

// slm_data_k4.hip
void launch_data_gram(const FrameDev*, int, int, double, int, hipStream_t, const int* reuse, int wgs, int n_cus);
void launch_begin_and_gram(const FrameDev*, int, double, hipStream_t, const int* reuse, int dag_cut, int wgs, int n_cus);
void launch_data_eval(const FrameDev*, int, int, double, int mode, hipStream_t, const int* reuse = nullptr);
void launch_band_assemble(const FrameDev*, int, int, hipStream_t);

// slm_front.hip
void launch_front_assemble(const FrameDev*, int, int, hipStream_t);
void launch_pair_reduce(const FrameDev*, int, int, hipStream_t);
void launch_pair_scatter(const FrameDev*, int, int, hipStream_t);
void launch_reg_grad_nd(const FrameDev*, int, int, int, double, int, double, hipStream_t);
void launch_front_load_rhs(const FrameDev*, int, int, hipStream_t);
void launch_iter_begin_nd(const FrameDev*, int, hipStream_t, const int* reuse, int dag_cut);
void launch_front_solve(const FrameDev*, int, const NDLevelSched*, int, double, hipStream_t);
void launch_front_levels(const FrameDev*, int, const NDLevelSched*, int, int, int, double, hipStream_t);

bool ensure_dynamic_lds(const void* kernel, size_t bytes);   // every kernel with more than 64 KB of dynamic LDS, before its launch

// slm_dag.hip
int launch_front_solve_dag(const FrameDev*, int, int, double, hipStream_t, int cut, bool reset, bool check);
int dag_device_setup(int dev, int* xcd8_out);
int dag_last_mode();
hipError_t set_dag_timeout_ticks(long long);
void launch_dag_abort_check(const FrameDev*, int, hipStream_t);

// slm_band.hip
void launch_bandwidth(const slm_frame&, int*, hipStream_t);
void launch_band_solve(const FrameDev*, int, int, int, double, hipStream_t);
void launch_band_to_dense(const FrameDev*, int, double*, hipStream_t);
void launch_dense_to_band(const FrameDev*, const double*, const double*, hipStream_t);

// slm_reg.hip
void launch_reg_grad(const FrameDev*, int, int, int, double, int, double, hipStream_t);
void launch_after_solve(const FrameDev*, int, int, int, int, double, int, double, int, hipStream_t);
void launch_reg_loss(const FrameDev*, int, int, int, double, int, double, int, hipStream_t);

// slm_misc.hip (the LM loop's state kernels)
void launch_init_slot(const FrameDev*, int, int, const slm_config&, hipStream_t);
void launch_iter_begin(const FrameDev*, int, hipStream_t);
void launch_pack_nodes(const FrameDev*, int, int, hipStream_t);
void launch_make_trial(const FrameDev*, int, int, hipStream_t);
void launch_pack_target(int, const float*, const float*, float4*, hipStream_t);
void launch_pack_target_px(int, const int*, const uint8_t*, const float*, const float*, float4*, hipStream_t);
void launch_accept(const FrameDev*, int, int, int, int, hipStream_t, int* reuse = nullptr, int eval_pass = 0);
void launch_loss_out(const FrameDev*, int, int, double*, hipStream_t);
// (a term's pairs at `part` and its nb kept counts at cnt_part or, with a FaceDev array, its mesh's triangle count)
struct FaceDev;
void launch_term_loss_out(const FrameDev*, int slot, int part, int nb, int cnt_part, const FaceDev* face, double* out, hipStream_t);
void launch_zero_reg_part(const FrameDev*, int, int, hipStream_t);
