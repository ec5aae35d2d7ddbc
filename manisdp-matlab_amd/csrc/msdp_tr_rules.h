// msdp_tr_rules.h -- the scalar decisions of Manopt's tCG.m and trustregions.m, stated once.
//
// The routes that run a tCG on the device -- the three-launch trips, the two-launch trip, the persistent kernel of the block
// kinds -- move their scalars through different plumbing (frames in global memory, registers) and take their decisions here.
// (msdp_persist.hip, msdp_pipe.h and msdp_trip1.hip still write the same expressions out: the register allocation of the first
// two and the measured trip of the third did not hold when the predicates became calls)  The predicates return the condition to GO ON and are negated at
// the call site: in that form the branches fold as the written-out tests did.
// The functions are pure: scalars in, scalars out; no memory access, no Dev, no Ctl, no thread index.  What is NOT here:
// bench_mode (the `!bench &&` in front of a predicate is the caller's; it is no rule of the algorithm), sqrt(r_r) (the caller
// forms norm_r, unconditionally, in front of its guard), the inner products themselves, and the loop bound of tCG.m:160: it is
// the bare comparison `j >= maxinner` behind the convergence test at every call site (the stop code stays 5), and a call in its
// place keeps the first control-flow simplification from folding the branch.
//
// No fp-contract pragma: the functions take the mode of the unit that includes them.  The persistent units pin
// `#pragma clang fp contract(on)` in front of their includes, and there the grouping below -- which products share an
// expression with their sum -- decides what fuses.  Do not regroup.
#pragma once

// ---- tCG.m:170-198: the step to the boundary
// <eta + alpha mdelta, eta + alpha mdelta>_P   (:173)
__device__ __forceinline__ double tcg_e_Pe_new(double e_Pe, double alpha, double e_Pd, double d_Pd) {
    return e_Pe + 2.0 * alpha * e_Pd + alpha * alpha * d_Pd;
}
// positive curvature and the trial step stays inside the trust region: the negation of the test of :183
__device__ __forceinline__ bool tcg_step_inside(double d_Hd, double e_Pe_new, double Delta) {
    return !(d_Hd <= 0.0 || e_Pe_new >= Delta * Delta);
}
// otherwise eta - tau mdelta lies on the boundary   (:188)
__device__ __forceinline__ double tcg_tau(double e_Pd, double d_Pd, double e_Pe, double Delta) {
    return (-e_Pd + sqrt(e_Pd * e_Pd + d_Pd * (Delta * Delta - e_Pe))) / d_Pd;
}
// and the stop code is 1 (negative curvature) or 2 (exceeded trust region)   (:194-198)
__device__ __forceinline__ int tcg_boundary_stop(double d_Hd) { return (d_Hd <= 0.0) ? 1 : 2; }

// ---- tCG.m:227-287: model check, convergence test, loop bound, recurrences
// the model decreased: the negation of the test of :228 (otherwise the trial step is dropped, stop 6)
__device__ __forceinline__ bool tcg_model_decreased(double new_model, double model_value) { return !(new_model >= model_value); }
// norm_r0 ^ theta of the convergence test, the same in every trip of a tCG   (:249)
__device__ __forceinline__ double tcg_nr0t(double norm_r0, double theta) { return (theta == 1.0) ? norm_r0 : pow(norm_r0, theta); }
// the residual is above its target norm_r0 min(norm_r0^theta, kappa), or trip mininner is not reached: the negation of the test
// of :249
__device__ __forceinline__ bool tcg_unconverged(int j, int mininner, double norm_r, double norm_r0, double nr0t, double kappa) {
    return !(j >= mininner && norm_r <= norm_r0 * fmin(nr0t, kappa));
}
// otherwise the stop code is 3 (linear, kappa) or 4 (superlinear, theta)   (:250-254)
__device__ __forceinline__ int tcg_converged_stop(double kappa, double nr0t) { return (kappa < nr0t) ? 3 : 4; }
// beta and the recurrences of <eta, mdelta>_P, <mdelta, mdelta>_P and <z, r>   (:272, :286, :287).  z_r_new is <r, r> without a
// preconditioner and <z, r> with one.  Returns beta.
__device__ __forceinline__ double tcg_recurrences(double z_r_new, double alpha, double& z_r, double& e_Pd, double& d_Pd) {
    const double beta = z_r_new / z_r;                      // :272
    e_Pd = beta * (e_Pd + alpha * d_Pd);                    // :286
    d_Pd = z_r_new + beta * beta * d_Pd;                    // :287
    z_r = z_r_new;
    return beta;
}

// ---- trustregions.m:548-729: rho, the new radius, accept or reject
// fx, fp: cost at the point and at the proposal; prd = <eta, grad + .5 Heta>; stop: how the tCG ended.  Delta: the radius, in
// and out.  Returns whether the proposal is accepted.
__device__ __forceinline__ bool rtr_outcome(double fx, double fp, double prd, double rho_reg_opt, double rho_prime,
                                            double Delta_bar, int stop, double& Delta, double& rho, double& rhonum, double& rhoden) {
    rhonum = fx - fp;                                                    // :548
    rhoden = -prd;                                                       // :550
    const double rho_reg = fmax(1.0, fabs(fx)) * 2.220446049250313e-16 * rho_reg_opt;   // :579
    rhonum += rho_reg;
    rhoden += rho_reg;
    const bool model_decreased = rhoden >= 0.0;                          // :614
    rho = rhonum / rhoden;                                               // :621
    if (rho < 0.25 || !model_decreased || isnan(rho)) Delta = Delta / 4.0;                      // :653
    else if (rho > 0.75 && (stop == 1 || stop == 2)) Delta = fmin(2.0 * Delta, Delta_bar);      // :669
    return model_decreased && rho > rho_prime;                           // :688
}
// stoppingcriterion.m:51-72
__device__ __forceinline__ bool rtr_done(double norm_grad, double tolgradnorm, int k, int maxiter) {
    return norm_grad < tolgradnorm || k >= maxiter;
}
