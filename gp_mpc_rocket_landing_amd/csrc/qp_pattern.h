// qp_pattern.h -- host analysis of a QP's sparsity pattern: which KKT factor layout the
// device uses for it (qp_device.h mode 0 / qp_block.h mode 1), the term lists of every factor
// slot, and the packed int block the kernels read.  Plain C++ with no device call, so that
// gpmpc_qp_pattern_info can answer on a machine without a GPU; QPPatternHost::build uploads
// what it returns.  Needs the caps and block sizes of qp.h / qp_device.h / qp_block.h
// (QP_NMAX, QP_W, QP_FAC_CAP, QP_BLK_SZ, QP_BLK_CM) defined before it is included.
#pragma once
#include <algorithm>
#include <cstddef>
#include <vector>

struct QPPatternPlan {
  int n = 0, m = 0, nnz = 0, w = 0, maxrow = 0, maxcol = 0;
  int mode = 0, fac_len = 0, nblk = 0, n_offd = -1;
  // one device block: rowptr | colidx | colptr | csc2csr | cscrow | facptr | facdiag | terms | offd
  std::vector<int> all;
  size_t o_rp = 0, o_ci = 0, o_cp = 0, o_cm = 0, o_cr = 0, o_bp = 0, o_fd = 0, o_tv = 0, o_od = 0;
};

// rowptr (m+1) and colidx (rowptr[m]) must be a well-formed CSR pattern with columns in [0, n)
inline QPPatternPlan qp_pattern_analyze(int n, int m, const int *rowptr, const int *colidx) {
  QPPatternPlan pl;
  pl.n = n;
  pl.m = m;
  const int nnz = pl.nnz = rowptr[m];
  int w = 0;
  for (int r = 0; r < m; ++r)
    for (int a = rowptr[r]; a < rowptr[r + 1]; ++a)
      for (int b = rowptr[r]; b < rowptr[r + 1]; ++b) w = std::max(w, colidx[a] - colidx[b]);
  pl.w = w;
  for (int r = 0; r < m; ++r) pl.maxrow = std::max(pl.maxrow, rowptr[r + 1] - rowptr[r]);
  // CSC map
  std::vector<int> colptr(n + 1, 0), csc2csr(nnz), cscrow(nnz);
  for (int k = 0; k < nnz; ++k) colptr[colidx[k] + 1]++;
  for (int j = 0; j < n; ++j) colptr[j + 1] += colptr[j];
  for (int j = 0; j < n; ++j) pl.maxcol = std::max(pl.maxcol, colptr[j + 1] - colptr[j]);
  std::vector<int> fill(colptr.begin(), colptr.end() - 1);
  for (int r = 0; r < m; ++r)
    for (int k = rowptr[r]; k < rowptr[r + 1]; ++k) {
      const int p = fill[colidx[k]]++;
      csc2csr[p] = k;
      cscrow[p] = r;
    }
  // Factor layout.  Mode 1 (block tridiagonal, qp_block.h) when every coupled
  // pair (i >= j) of M = P + A'RA lies in one block of QP_BLK_SZ variables or
  // in neighbouring blocks with i among the first QP_BLK_CM rows of its block
  // (the MPC stage structure); otherwise mode 0, the banded LDL^T with column
  // stride QP_W+1.  Either way every LDS slot gets its list of rho_r A[a] A[b]
  // terms, generated in (row, a, b) order like the C oracle's factor().
  constexpr int NB = QP_W + 1, SZ = QP_BLK_SZ, CM = QP_BLK_CM, BS = SZ * SZ + SZ * CM;
  const int nblk = pl.nblk = (n + SZ - 1) / SZ;
  bool blk = true;
  for (int r = 0; r < m && blk; ++r)
    for (int a = rowptr[r]; a < rowptr[r + 1]; ++a)
      for (int b = rowptr[r]; b < rowptr[r + 1]; ++b) {
        const int i = colidx[a], j = colidx[b];
        if (j > i) continue;
        const int bi = i / SZ, bj = j / SZ;
        if (!(bi == bj || (bi == bj + 1 && i - bi * SZ < CM))) blk = false;
      }
  if (blk && nblk * BS - SZ * CM > QP_FAC_CAP) blk = false;
  // a block-structured pattern whose whole blocks pass the variable cap (n = 211..216: the
  // last block's identity pad rows would not fit) is banded too, and takes mode 0 if it fits
  if (blk && nblk * SZ > QP_NMAX && w <= QP_W && n * NB <= QP_FAC_CAP) blk = false;
  pl.mode = blk ? 1 : 0;
  const int fac_len = pl.fac_len = blk ? nblk * BS - SZ * CM : n * NB;
  struct T { int e, r, a, b; };
  std::vector<T> terms;
  std::vector<int> facdiag(fac_len, -1);
  for (int r = 0; r < m; ++r)
    for (int a = rowptr[r]; a < rowptr[r + 1]; ++a)
      for (int b = rowptr[r]; b < rowptr[r + 1]; ++b) {
        const int i = colidx[a], j = colidx[b];
        if (j > i) continue;
        if (!blk) {
          terms.push_back(T{j * NB + (i - j), r, a, b});
          continue;
        }
        const int bi = i / SZ, bj = j / SZ, ri = i - bi * SZ, rj = j - bj * SZ;
        if (bi == bj) {
          terms.push_back(T{bi * BS + rj * SZ + ri, r, a, b});
          if (i != j) terms.push_back(T{bi * BS + ri * SZ + rj, r, a, b});
        } else {
          terms.push_back(T{bj * BS + SZ * SZ + rj * CM + ri, r, a, b});
        }
      }
  if (blk) {
    for (int v = 0; v < nblk * SZ; ++v) {
      const int k = v / SZ, rv = v - k * SZ;
      facdiag[k * BS + rv * SZ + rv] = (v < n) ? v : -2;  // identity rows pad the last block
    }
  } else {
    for (int j = 0; j < n; ++j) facdiag[j * NB] = j;
  }
  std::stable_sort(terms.begin(), terms.end(), [](const T &x, const T &y) { return x.e < y.e; });
  std::vector<int> facptr(fac_len + 1, 0), tv(3 * terms.size());
  for (size_t k = 0; k < terms.size(); ++k) {
    facptr[terms[k].e + 1]++;
    tv[3 * k] = terms[k].r;
    tv[3 * k + 1] = terms[k].a;
    tv[3 * k + 2] = terms[k].b;
  }
  for (int e = 0; e < fac_len; ++e) facptr[e + 1] += facptr[e];
  // mode 1: the non-diagonal slots that are not plain zeros, one int4 each
  // (QPPattern::offd), so the fleet's assembly reads one coalesced item per
  // slot instead of walking facdiag / facptr / terms for every slot
  std::vector<int> offd;
  int n_offd = -1;
  if (blk && fac_len < (1 << 15) && nnz < (1 << 16)) {
    n_offd = 0;
    for (int e = 0; e < fac_len && n_offd >= 0; ++e) {
      if (facdiag[e] >= 0) continue;
      const int k0 = facptr[e], k1 = facptr[e + 1], one = facdiag[e] == -2;
      if (k1 == k0 && !one) continue;
      if (k1 - k0 > 3) { n_offd = -1; break; }
      int it[4] = {e | (one << 15) | ((k1 - k0) << 16), 0, 0, 0};
      for (int k = k0; k < k1; ++k) it[1 + k - k0] = tv[3 * k + 1] | (tv[3 * k + 2] << 16);
      offd.insert(offd.end(), it, it + 4);
      ++n_offd;
    }
  }
  if (n_offd < 0) offd.clear();
  pl.n_offd = n_offd;
  std::vector<int> &all = pl.all;
  auto app = [&](const int *p, size_t k) { all.insert(all.end(), p, p + k); };
  pl.o_rp = 0;
  app(rowptr, m + 1);
  pl.o_ci = all.size();
  app(colidx, nnz);
  pl.o_cp = all.size();
  app(colptr.data(), n + 1);
  pl.o_cm = all.size();
  app(csc2csr.data(), nnz);
  pl.o_cr = all.size();
  app(cscrow.data(), nnz);
  pl.o_bp = all.size();
  app(facptr.data(), facptr.size());
  pl.o_fd = all.size();
  app(facdiag.data(), facdiag.size());
  pl.o_tv = all.size();
  app(tv.data(), tv.size());
  while (all.size() % 4) all.push_back(0);  // int4 alignment (the buffer itself is 256-B aligned)
  pl.o_od = all.size();
  app(offd.data(), offd.size());
  return pl;
}
