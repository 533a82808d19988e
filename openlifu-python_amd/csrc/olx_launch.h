// Launchers of the kernel-2 families, one translation unit each (k_*.hip).  Each enqueues ONE launch of the
// planned variant on the context's stream, writing |p| to `pm` (the current output buffer) and the other planned
// outputs to the context's buffers; errors surface through hipGetLastError in olx_field_launch.
#pragma once
struct olx_ctx;
// The operands and block records one launch of kernels 2e / 2f / 2g works through: all of them, or one side of a launch split at
// fp8_kcut (olx_field_launch: e4m3 correction products from the cut on, three fp16 products below it, operands bfrag_half / afrag_half on)
struct LatticePart { const uint4* bfrag; uint4* afrag /*olx_pack_toep writes it*/; const CosetBlock* blocks; unsigned n_blocks; bool fp8; };
void olx_launch_accum(olx_ctx* c, float* pm);        // 2a  field_accum_k
void olx_launch_accum_dir(olx_ctx* c, float* pm);    // 2a-d field_accum_dir_k (piston directivity; needs c->d_tab2)
bool olx_launch_shared(olx_ctx* c, float* pm);       // 2b  field_shared_k (false: no instantiation for the planned shape)
void olx_launch_mfma(olx_ctx* c, float* pm);         // 2c  field_mfma_k
void olx_launch_lattice(olx_ctx* c, float* pm);      // 2d  field_lattice_k
void olx_launch_coset(olx_ctx* c, const LatticePart& q, float* pm);    // 2e  field_coset_k
void olx_launch_cosetp(olx_ctx* c, const LatticePart& q, float* pm);   // 2g  field_cosetp_k (2e's NT = 2 shape, planes in the MFMA rows)
void olx_launch_toep(olx_ctx* c, const LatticePart& q, float* pm);     // 2f  field_toep_k (single steering column on a lattice array)
void olx_pack_toep(olx_ctx* c, const LatticePart& q);                  //     its Toeplitz weight fragments (into q.afrag, e4m3 pieces with q.fp8)
void olx_launch_hetero(olx_ctx* c, float* pm);       // 2h  field_hetero_k
void olx_launch_hmarch(olx_ctx* c, float* pm);       // 2m  field_hmarch_k (marched ray sums: one launch per plane segment)
void olx_pack_hetero(olx_ctx* c);                    //     its steering table (c->nf foci per launch tile)
void olx_launch_pulse(olx_ctx* c, float* pm);       // 2p  field_pulse_k (pulsed model, olx_field_pulse; writes p_min to pm; the RESP instantiations when the plan carries olx_field_pulse_response)
void olx_launch_pulse_trace(olx_ctx* c, int n_points);   // 2p  field_pulse_k<false, true, RESP>: p(t_k) at the n_points voxels of c->d_ptrace_vox into c->d_ptrace (zeroed on the stream by the caller)
void olx_launch_pulse_med(olx_ctx* c, float* pm);   // 2ph field_pulse_med_k (pulsed model through a medium, olx_field_pulse_medium; all foci in one wave per voxel)
void olx_launch_pulse_med_trace(olx_ctx* c, int n_points);   // 2ph field_pulse_med_k<R, false, true>: as olx_launch_pulse_trace
void olx_launch_bfmed(olx_ctx* c, int n_foci);      // 1m  bf_med_k (StraightRay delays into the steering table; after bf_solve_k)
void olx_launch_bfapod(olx_ctx* c, int n_foci, int mode, int spreading, bool with_delays);   // 1a  bf_med_k<SIG, true> (MediumCompensated apodization; with_delays: one walk with 1m's delays)
void olx_launch_steer_table(olx_ctx* c, const double* apertures, double wscale, double inv_2lambda);   // 4  steer_table_k (element records into c->d_sm_tabd / d_sm_tabf; apertures = { xaxis [N][3], size [N][2] } on the device, or null)
void olx_launch_steer_map(olx_ctx* c, const SteerParams& P, int kind, bool directivity);                   // 4  steer_map_k (P and n_active into c->d_sm_p / d_sm_n)
void olx_launch_steer_map_medium(olx_ctx* c, const SteerMedParams& M, int kind, int comp /* 0 none, 1 equalize, 2 matched */, bool phase, bool directivity);   // 4h steer_map_med_k (P and n_active into c->d_smm_p / d_smm_n)
void olx_thermal_pack(olx_ctx* c, const float* rho, const float* cp, const float* kap, const float* alpha);   // 3  thermal_pack_k (coefficients, FTCS rate)
void olx_thermal_step(olx_ctx* c, const float* inten, int step, const ThermalStep& S);                        // 3  thermal_step_k (one step)
void olx_thermal_trace_last(olx_ctx* c, int step);                                                          //    thermal_trace_k (last trace row)
void olx_fullwave_pack(olx_ctx* c, const float* cs, const float* rho, const float* alpha);   // 5  fullwave_pack_k (coefficient volumes of a heterogeneous medium)
void olx_fullwave_step(olx_ctx* c, int step, bool pii);                                      // 5  fullwave_inject_k | fullwave_inject_elem_k, fullwave_vel_k, fullwave_pres_k, fullwave_trace_k (one step)
void olx_fullwave_aperture_weights(olx_ctx* c, int n_el, long long max_box, long long total);   // 5  fullwave_aperture_k (dense weights of every element's index box)
void olx_fullwave_drive_fill(olx_ctx* c);                                                    // 5  fullwave_drive_k (the drive table of the element-factored sources; with a response: the extended bare table, then fullwave_drive_fir_k)
void olx_eikonal_init(olx_ctx* c, const float* cs);                      // 6  eikonal_init_k (the init set into both c->d_ek_T; cs = the device sound-speed volume, or null: uniform c->ek.c0)
void olx_eikonal_sweep(olx_ctx* c, const float* cs, int sweep);          // 6  eikonal_sweep_k (Jacobi sweep number `sweep` >= 1 over its box; its flag is c->d_ek_flag[sweep - 1])
void olx_eikonal_sample_launch(olx_ctx* c, int n_points, int n_entries); // 6  eikonal_sample_k (the CSR table of c->d_ek_row / d_ek_vox / d_ek_w into c->d_ek_out)
