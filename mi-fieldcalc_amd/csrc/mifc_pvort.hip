// mifc_pvort.hip -- Ertel potential vorticity of level batches (mifc_pvort_hlevels / mifc_pvort_fields /
// mifc_pvort_levels, include/mifc.h; EXTENSION: the reference has no function that crosses levels).
//
// The first kernel here that differences a batch along all three axes in one walk.  A workgroup owns a tile of
// PVORT_TILE_ROWS interior rows by PVORT_LANES_X * V columns and walks the levels once, as vderiv_kernel does
// (mifc_vderiv.hip): a lane keeps its V cells of u, v, th and the coordinate for the levels k - 1, k and k + 1 in
// rotating slots, the loads run two levels ahead of the level being stored, output level k is stored as soon as level
// k + 1 has arrived.  The row and column neighbours of level k come from LDS: every lane puts its cells of level k into
// the tile of the level (two tiles, alternating, so that a level costs one barrier), 160 lanes also fetch one piece of
// the tile's halo each -- the row above and the row below for u and th, the column to the left and to the right for v
// and th -- through the same rotating slots, so a halo row is fetched from L2 or HBM as early as the lane's own cells.
// The tiles cover interior rows only; the lane of row 1 also stores row 0 and the lane of row ny - 2 row ny - 1, in x the
// ring cells sit in the lane of their interior neighbour (V = 4) or are stored by it (V = 1): the ring is a copy
// (fillEdges).  No address leaves the planes: a halo index is clamped into the row, lanes past the tile's end walk the
// tile's first cells and neither store nor count.
// The vertical derivatives are the double r of mifc_vderiv_* before its rounding, from the one statement of its rules
// that vderiv_kernel uses too (mifc_vderiv_cell.h; the coordinate of a level: mifc_column_walk.h), by the same two bodies: where every
// interior cell of the wave has both sides for all three fields and eight defined neighbours -- one ballot -- the fast
// body runs without a select, the general body does the rest.  Undefined interior cells are counted per level by ballot
// into one LDS word per tile buffer and leave the workgroup as one atomic per level that has something to count (DESIGN.md
// 4.8, 4.17c): no limit on nlev follows.
#include "mifc_kernels.h"
#include "mifc_vderiv_cell.h"

namespace mifc {

namespace {

constexpr int LX = PVORT_LANES_X, TY = PVORT_TILE_ROWS;
constexpr int FU = 0, FV = 1, FT = 2;
const unsigned int LANE_COUNTED = 4 /* bits 0 .. 3: the cell is inside */, LANE_ACTIVE = 1u << 8, LANE_STORE_SELF = 1u << 9, LANE_STORE_FIRST = 1u << 10, LANE_STORE_LAST = 1u << 11,
                   LANE_ROW_BEGIN = 1u << 12, LANE_ROW_END = 1u << 13, LANE_HALO_ROW = 1u << 14, LANE_HALO_COLUMN = 1u << 15;

template <int KIND, int V>
__global__ __launch_bounds__(256, 2) void pvort_kernel(const PvortParams P)
{
  constexpr int R = 3, NF = 3;
  constexpr int TX = LX * V;
  constexpr int PITCH = TX + 8;           // a lane's cells from column 4 on (16-byte grid), the halo columns at 3 and 4 + columns
  constexpr int PLANE = (TY + 2) * PITCH; // the halo row above, the tile's rows, the halo row below
  __shared__ __attribute__((aligned(16))) float s_tile[2][NF][PLANE];
  __shared__ unsigned int s_cnt[2];
  static_assert(4 * LX + 4 * TY <= 256 && LX * TY == 256, "one halo piece per lane at most");

  const int nx = P.nx, nlev = P.nlev, method = P.method;
  const int t = threadIdx.x, lx = t & (LX - 1), ly = t / LX;
  const int xt0 = (int)blockIdx.x * TX, y0 = P.c0 + (int)blockIdx.y * TY;
  const int cols_here = min(TX, nx - xt0), rows_here = min(TY, P.c1 - y0 + 1);
  const int x0 = xt0 + lx * V, y = y0 + ly;
  const bool active = x0 < nx && ly < rows_here; // (V = 4: nx % 4 == 0, a lane is inside with all four cells or with none)
  // lanes past the tile's end walk its first cells
  const int own_off = active ? (y - P.g0) * nx + x0 : (y0 - P.g0) * nx + xt0;
  const int own_lds = (ly + 1) * PITCH + 4 + lx * V;
  if (t < 2)
    s_cnt[t] = 0;

  // the lane's piece of the halo: 1 = V cells of a row, 2 = one cell of a column
  int h_kind = 0, h_off = 0, h_lds = 0, h_field = 0;
  if (t < 4 * LX) {
    const int below = t / (2 * LX), hx0 = xt0 + lx * V;
    if (hx0 < nx) {
      const int row = below ? y0 + rows_here : y0 - 1; // c0 - 1 <= row <= c1 + 1: inside the planes
      h_kind = 1;
      h_off = (row - P.g0) * nx + hx0;
      h_lds = (below ? rows_here + 1 : 0) * PITCH + 4 + lx * V;
      h_field = ((t / LX) & 1) ? FT : FU;
    }
  } else if (t < 4 * LX + 4 * TY) {
    const int j = t - 4 * LX, r = j % TY, right = (j / TY) & 1;
    if (r < rows_here) {
      const int gx = right ? min(xt0 + cols_here, nx - 1) : max(xt0 - 1, 0); // clamped into the row
      h_kind = 2;
      h_off = (y0 + r - P.g0) * nx + gx;
      h_lds = (r + 1) * PITCH + (right ? 4 + cols_here : 3);
      h_field = j / (2 * TY) ? FT : FV;
    }
  }
  const float* const h_base = h_field == FU ? P.u : (h_field == FV ? P.v : P.th);

  // the cells that are computed, stored and counted as themselves
  unsigned int inside = 0;
#pragma unroll
  for (int c = 0; c < V; ++c)
    inside |= (active && x0 + c >= 1 && x0 + c <= nx - 2) ? 1u << c : 0u;
  // What the lane is, in one word that is looked at where it is used (as lane masks these tests sat in SGPRs through the
  // walk, 24 to 31 of them spilled): bit c = cell c is inside, LANE_COUNTED + c = and counted here (a row computed for
  // the ring alone is counted by the band that owns it), the rows it stores, its place in the row, its piece of the halo.
  const bool self = y >= P.own0 && y < P.own1;
  const unsigned int lane_word = inside | (self ? inside << LANE_COUNTED : 0u) | (active ? LANE_ACTIVE : 0u) | (active && self ? LANE_STORE_SELF : 0u) |
                                 (active && y == 1 && P.own0 == 0 ? LANE_STORE_FIRST : 0u) | (active && y == P.ny - 2 && P.own1 == P.ny ? LANE_STORE_LAST : 0u) |
                                 (x0 == 0 ? LANE_ROW_BEGIN : 0u) | (x0 + V == nx ? LANE_ROW_END : 0u) | (h_kind == 1 ? LANE_HALO_ROW : 0u) |
                                 (h_kind == 2 ? LANE_HALO_COLUMN : 0u);

  const float undef = P.undef;
  const ConstFloats ab = (ConstFloats)(unsigned long long)P.ab;
  const ConstWords lev_bits = (ConstWords)(unsigned long long)P.lev_bits;
  const ConstDoubles lev_w = (ConstDoubles)(unsigned long long)P.lev_w;
  typedef WalkLevel<NF, V> Level;

  auto load = [&](Level& L, float (&h)[V], int k) {
    const long off = (long)walk_here(k) * P.stride; // (k opaque: no induction variable per pointer)
    if constexpr (KIND == VDERIV_FIELD)
      walk_load<V>(L.c, P.coord + off + own_off);
    walk_load<V>(L.x[FU], P.u + off + own_off);
    walk_load<V>(L.x[FV], P.v + off + own_off);
    walk_load<V>(L.x[FT], P.th + off + own_off);
    const unsigned int lane = walk_here_v(lane_word);
    if ((lane & LANE_HALO_ROW) != 0)
      walk_load<V>(h, h_base + off + h_off);
    else if ((lane & LANE_HALO_COLUMN) != 0)
      h[0] = h_base[off + h_off];
  };
  // level k into the tile `buf`
  auto share = [&](const Level& L, const float (&h)[V], int buf) {
    const unsigned int lane = walk_here_v(lane_word);
    if ((lane & LANE_ACTIVE) != 0) {
#pragma unroll
      for (int f = 0; f < NF; ++f) {
        float* p = &s_tile[buf][f][own_lds];
        if constexpr (V == 4)
          *reinterpret_cast<float4*>(p) = make_float4(L.x[f][0], L.x[f][1], L.x[f][2], L.x[f][3]);
        else
          p[0] = L.x[f][0];
      }
    }
    if ((lane & LANE_HALO_ROW) != 0) {
      float* p = &s_tile[buf][h_field][h_lds];
      if constexpr (V == 4)
        *reinterpret_cast<float4*>(p) = make_float4(h[0], h[1], h[2], h[3]);
      else
        p[0] = h[0];
    } else if ((lane & LANE_HALO_COLUMN) != 0) {
      s_tile[buf][h_field][h_lds] = h[0];
    }
  };

  // what does not depend on the level: the map ratios and the Coriolis parameter of the lane's cells, ps
  float xm[V], ym[V], fc[V], ps[V];
  walk_load<V>(xm, P.xmapr + own_off);
  walk_load<V>(ym, P.ymapr + own_off);
  const bool has_f = P.fcoriolis != nullptr;
#pragma unroll
  for (int c = 0; c < V; ++c)
    fc[c] = ps[c] = 0.f;
  if (has_f)
    walk_load<V>(fc, P.fcoriolis + own_off);
  if constexpr (KIND == VDERIV_HYBRID) {
    walk_load<V>(ps, P.coord + own_off);
    walk_usable_ps<V>(ps, P.ps_all != 0, undef); // a coordinate that is not usable is carried as NaN (rule 1)
  }

  // stores level k; a row of the output at `row` (a grid row)
  auto store_row = [&](const float (&res)[V], int k, int row, unsigned int lane) {
    float* p = P.out + (long)walk_here(k) * P.stride + (long)(row - P.g0) * nx;
    if constexpr (V == 4) {
      *reinterpret_cast<float4*>(p + x0) = make_float4(res[0], res[1], res[2], res[3]);
    } else {
      if ((lane & 1u) != 0) {
        p[x0] = res[0];
        if (x0 == 1)
          p[0] = res[0];
        if (x0 == nx - 2)
          p[nx - 1] = res[0];
      }
    }
  };

  // Output level k from the levels k - 1 (lo), k (cur) and k + 1 (hi), their coordinates cp, cc, cn and the words of
  // vderiv_defined dfp, dfk, dfn; the halo piece h of level k.
  auto level = [&](const Level& lo, const Level& cur, const Level& hi, const float (&h)[V], const float (&cp)[V], const float (&cc)[V],
                   const float (&cn)[V], const unsigned int (&dfp)[V], const unsigned int (&dfk)[V], const unsigned int (&dfn)[V],
                   unsigned int bits_k, int k) {
    const int buf = k & 1;
    const unsigned int lane = walk_here_v(lane_word);
    share(cur, h, buf);
    __syncthreads(); // level k of the tile is complete; the tile of level k - 1 may be overwritten by the next level
    if (t == 0 && k > 0) {
      // the counts of level k - 1 are complete too
      const unsigned int n = s_cnt[buf ^ 1];
      if (n != 0) {
        atomicAdd(P.n_undefined + (k - 1), (u64)n);
        s_cnt[buf ^ 1] = 0;
      }
    }

    // rule 3: the neighbours of level k, tested, and their float differences
    float dv[V], du[V], dtx[V], dty[V];
    unsigned int nb_ok = 0; // bit c: the eight neighbours of cell c are defined
    {
      const float* pv = &s_tile[buf][FV][own_lds];
      const float* pt = &s_tile[buf][FT][own_lds];
      const float* pu = &s_tile[buf][FU][own_lds];
      const float v_left = pv[-1], v_right = pv[V], t_left = pt[-1], t_right = pt[V];
      float uu[V], ud[V], tu[V], td[V];
      walk_load<V>(uu, pu - PITCH);
      walk_load<V>(ud, pu + PITCH);
      walk_load<V>(tu, pt - PITCH);
      walk_load<V>(td, pt + PITCH);
      const bool all_u = (bits_k & 1u) != 0, all_v = (bits_k & 2u) != 0, all_t = (bits_k & 4u) != 0;
#pragma unroll
      for (int c = 0; c < V; ++c) {
        const float vl = c > 0 ? cur.x[FV][c > 0 ? c - 1 : 0] : v_left, vr = c < V - 1 ? cur.x[FV][c < V - 1 ? c + 1 : 0] : v_right;
        const float tl = c > 0 ? cur.x[FT][c > 0 ? c - 1 : 0] : t_left, tr = c < V - 1 ? cur.x[FT][c < V - 1 ? c + 1 : 0] : t_right;
        const bool ok_u = all_u || all_def(undef, uu[c], ud[c]), ok_v = all_v || all_def(undef, vl, vr), ok_t = all_t || all_def(undef, tl, tr, tu[c], td[c]);
        nb_ok |= ((ok_u && ok_v && ok_t) || ((lane >> c) & 1u) == 0) ? 1u << c : 0u;
        dv[c] = vr - vl;
        du[c] = ud[c] - uu[c];
        dtx[c] = tr - tl;
        dty[c] = td[c] - tu[c];
      }
      nb_ok = walk_here_v(nb_ok);
    }

    // rules 1 and 3 of mifc_vderiv_* for the coordinate, then the sides of every field (mifc_vderiv_cell.h)
    const bool weighted = walk_here(method) != 0;
    unsigned int cm[V];
    double h1[V], h2[V], den[V];
    vderiv_cell_mask<KIND, V>(cm, h1, h2, den, cp, cc, cn, bits_k, weighted);
    unsigned int cls[V];
    unsigned int every = SIDE_BOTH, any = 0;
#pragma unroll
    for (int c = 0; c < V; ++c)
      cls[c] = vderiv_classify<NF>(every, any, cm[c], dfp[c], dfk[c], dfn[c], ((lane >> c) & 1u) != 0);
    const bool good = every == SIDE_BOTH && nb_ok == (1u << V) - 1u;

    // rules 3 to 5 of this entry for one cell from its derivatives
    const double scale = P.scale;
    auto product = [&](int c, double Du, double Dv, double Dt) -> float {
      const double hx = 0.5 * (double)xm[c], hy = 0.5 * (double)ym[c];
      const double dxv = hx * (double)dv[c], dyu = hy * (double)du[c], dxt = hx * (double)dtx[c], dyt = hy * (double)dty[c];
      const double zeta = dxv - dyu;
      const double plus = zeta + (double)fc[c];
      const double za = has_f ? plus : zeta;
      const double t1 = za * Dt, t2 = Dv * dxt, t3 = Du * dyt;
      const double S = (t1 - t2) + t3;
      return (float)(scale * S);
    };

    float res[V];
    if (__builtin_amdgcn_ballot_w64(!good) == 0) {
      // the fast body: both sides and defined neighbours everywhere in the wave
#pragma unroll
      for (int c = 0; c < V; ++c) {
        double wa, wb, D[NF];
        vderiv_both_weights<KIND>(wa, wb, h1[c], h2[c], den[c], weighted, lev_w, k);
#pragma unroll
        for (int f = 0; f < NF; ++f)
          D[f] = vderiv_both(lo.x[f][c], cur.x[f][c], hi.x[f][c], wa, wb, weighted);
        res[c] = product(c, D[FU], D[FV], D[FT]);
      }
    } else {
      // the general body: only the weights that some cell of the wave needs
      const bool need_lower = __builtin_amdgcn_ballot_w64((any & (1u << (SIDE_LOWER - 1))) != 0) != 0;
      const bool need_upper = __builtin_amdgcn_ballot_w64((any & (1u << (SIDE_UPPER - 1))) != 0) != 0;
      const bool need_both = __builtin_amdgcn_ballot_w64((any & (1u << (SIDE_BOTH - 1))) != 0) != 0;
      unsigned int n_bad = 0;
#pragma unroll
      for (int c = 0; c < V; ++c) {
        double wl = 0.0, wh = 0.0, wa = 0.0, wb = 0.0, D[NF];
        if (need_lower)
          wl = vderiv_one_weight<KIND, false>(h1[c], lev_w, k);
        if (need_upper)
          wh = vderiv_one_weight<KIND, true>(h2[c], lev_w, k);
        if (need_both)
          vderiv_both_weights<KIND>(wa, wb, h1[c], h2[c], den[c], weighted, lev_w, k);
#pragma unroll
        for (int f = 0; f < NF; ++f)
          D[f] = vderiv_sided((cls[c] >> (2 * f)) & 3u, lo.x[f][c], cur.x[f][c], hi.x[f][c], wl, wh, wa, wb, weighted);
        const float r = product(c, D[FU], D[FV], D[FT]);
        const bool bad = ((cls[c] & 3u) == 0 || ((cls[c] >> 2) & 3u) == 0 || ((cls[c] >> 4) & 3u) == 0 || ((nb_ok >> c) & 1u) == 0);
        res[c] = bad ? undef : r;
        n_bad += (unsigned int)__popcll(__builtin_amdgcn_ballot_w64(bad && ((lane >> (LANE_COUNTED + c)) & 1u) != 0));
      }
      if (n_bad != 0 && (walk_here_v((unsigned int)t) & 63) == 0)
        atomicAdd(&s_cnt[buf], n_bad);
    }

    // the ring is a copy of its interior neighbour (fillEdges)
    if constexpr (V == 4) {
      res[0] = (lane & LANE_ROW_BEGIN) != 0 ? res[1] : res[0];
      res[3] = (lane & LANE_ROW_END) != 0 ? res[2] : res[3];
    }
    if ((lane & LANE_STORE_SELF) != 0)
      store_row(res, k, y, lane);
    if ((lane & LANE_STORE_FIRST) != 0)
      store_row(res, k, 0, lane);
    if ((lane & LANE_STORE_LAST) != 0)
      store_row(res, k, P.ny - 1, lane);
  };

  const float nan = __int_as_float(0x7fc00000);
  Level L[R], prev;
  float H[R][V];
#pragma unroll
  for (int c = 0; c < V; ++c) {
    prev.c[c] = L[2].c[c] = 0.f;
    H[0][c] = H[1][c] = H[2][c] = 0.f;
#pragma unroll
    for (int f = 0; f < NF; ++f)
      prev.x[f][c] = L[2].x[f][c] = 0.f;
  }
  load(L[0], H[0], 0);
  load(L[1], H[1], 1);
  if (2 < nlev)
    load(L[2], H[2], 2);

  unsigned int bits_k = lev_bits[0];
  float cp[V], cc[V];
  unsigned int dfp[V], dfk[V];
#pragma unroll
  for (int c = 0; c < V; ++c) {
    cp[c] = nan;
    dfp[c] = 0;
  }
  walk_coordinate<KIND, V>(cc, L[0].c, ps, ab, nlev, 0, bits_k, undef);
  vderiv_defined<NF, V>(dfk, L[0], bits_k, undef);

  for (int k0 = 0; k0 < nlev; k0 += R) {
#pragma unroll
    for (int d = 0; d < R; ++d) {
      const int k = k0 + d; // the output level
      if (k < nlev) {
        Level& cur = L[d];
        Level& nxt = L[(d + 1) % R];
        const bool has_next = k + 1 < nlev;
        const unsigned int bits_n = lev_bits[has_next ? k + 1 : k];
        float cn[V];
        walk_coordinate<KIND, V>(cn, nxt.c, ps, ab, nlev, has_next ? k + 1 : k, bits_n, undef);
#pragma unroll
        for (int c = 0; c < V; ++c)
          cn[c] = has_next ? cn[c] : nan;
        unsigned int dfn[V];
        vderiv_defined<NF, V>(dfn, nxt, bits_n, undef); // (no level k + 1: cn is NaN)
        level(prev, cur, nxt, H[d], cp, cc, cn, dfp, dfk, dfn, bits_k, k);
        // level k becomes level k - 1, level k + 1 level k; level k's slot takes level k + 3
        prev = cur;
        bits_k = bits_n;
#pragma unroll
        for (int c = 0; c < V; ++c) {
          cp[c] = cc[c];
          cc[c] = cn[c];
          dfp[c] = dfk[c];
          dfk[c] = dfn[c];
        }
        if (k + R < nlev)
          load(cur, H[d], k + R);
      }
    }
  }

  __syncthreads();
  if (t == 0) {
    const unsigned int n = s_cnt[(nlev - 1) & 1];
    if (n != 0)
      atomicAdd(P.n_undefined + (nlev - 1), (u64)n);
  }
}

template <int KIND>
hipError_t launch_v(const PvortParams& P, hipStream_t stream)
{
  const int tx = LX * (P.vec4 ? 4 : 1);
  const dim3 grid((unsigned int)((P.nx + tx - 1) / tx), (unsigned int)((P.c1 - P.c0 + TY) / TY)), block(256);
  if (P.vec4)
    hipLaunchKernelGGL((pvort_kernel<KIND, 4>), grid, block, 0, stream, P);
  else
    hipLaunchKernelGGL((pvort_kernel<KIND, 1>), grid, block, 0, stream, P);
  return hipGetLastError();
}

} // namespace

hipError_t launch_pvort(const PvortParams& P, hipStream_t stream)
{
  // every row the kernel touches lies in the planes of the launch
  if (P.nlev < 2 || P.nx < 3 || P.ny < 3 || P.c0 < 1 || P.c1 > P.ny - 2 || P.c0 > P.c1 || P.g0 < 0 || P.g0 > P.c0 - 1 || P.c1 + 1 > P.g0 + P.rows - 1 ||
      P.own0 < P.g0 || P.own1 > P.g0 + P.rows || P.own0 >= P.own1 || P.own1 > P.ny || (P.vec4 && ((P.nx & 3) != 0 || (P.stride & 3) != 0)) ||
      (long)P.rows * (long)P.nx > P.stride || (long)P.rows * (long)P.nx > 0x7fffffffL)
    return hipErrorInvalidValue;
  switch (P.kind) {
  case VDERIV_HYBRID:
    return launch_v<VDERIV_HYBRID>(P, stream);
  case VDERIV_FIELD:
    return launch_v<VDERIV_FIELD>(P, stream);
  case VDERIV_LEVELS:
    return launch_v<VDERIV_LEVELS>(P, stream);
  default:
    return hipErrorInvalidValue;
  }
}

} // namespace mifc
