// R12: Lanczos SVD of the prepared operator (raw and uncentred: quirk Q1) -- svd_las2 call sites
// /root/reference/src/dimred/pca/sparse/mod.rs:134-144, sparse_masked/mod.rs:316-331.
#pragma once
#include "engine.h"

namespace sapca {
// Fills h.sing (k values) and h.components_dev (k x n_used, sign-fixed) from h.a_used / h.at_used.
// centred (sapca_options.lanczos_center, opt-in): of A_c = A - 1 mu^T instead, mu = h.lz_mu (f64 means of the operator's
// columns over the global row count, in place on h.stream); the centring is fused into the products (lanczos.hip).
template <typename T>
void lanczos_fit(sapca_handle_s& h, bool centred = false);
}  // namespace sapca
