// The loop terms of the partition-function kernels (ensemble_kernels.hip, unpaired_kernels.hip): the small Turner-2004 tables
// staged in LDS as integers (0.01 kcal/mol) and the terms of oracle/lfold.c on them.  A Boltzmann factor is exp(EN_G * energy).
#pragma once
#include <hip/hip_runtime.h>
#include "fold_device.h"

namespace {

constexpr double EN_KT = 1.98717 * 310.15 / 1000.0;
constexpr double EN_G = -1.0 / (100.0 * EN_KT);

struct EnTables {
    int stack[8][8], bulge[31], internal_loop[31];
    int mismatchI[8][5][5], mismatchH[8][5][5], mismatchM[8][5][5], mismatch1nI[8][5][5], mismatch23I[8][5][5], mismatchExt[8][5][5];
    int dangle5[8][5], dangle3[8][5];
    int ML_closing, ML_intern, TerminalAU, ninio, MAX_NINIO;
};

__device__ __forceinline__ int en_off(int n, int d) { return d * n - ((d * (d - 1)) >> 1); }

__device__ inline void en_stage(EnTables* T, unsigned char* S, const FoldParams* __restrict__ P, const unsigned char* __restrict__ codes, int n, int tid, int nt) {
    for (int x = tid; x < 64; x += nt) T->stack[x >> 3][x & 7] = P->stack[x >> 3][x & 7];
    for (int x = tid; x < 31; x += nt) { T->bulge[x] = P->bulge[x]; T->internal_loop[x] = P->internal_loop[x]; }
    for (int x = tid; x < 200; x += nt) {
        const int t = x / 25, a = (x % 25) / 5, b = x % 5;
        T->mismatchI[t][a][b] = P->mismatchI[t][a][b]; T->mismatchH[t][a][b] = P->mismatchH[t][a][b]; T->mismatchM[t][a][b] = P->mismatchM[t][a][b];
        T->mismatch1nI[t][a][b] = P->mismatch1nI[t][a][b]; T->mismatch23I[t][a][b] = P->mismatch23I[t][a][b]; T->mismatchExt[t][a][b] = P->mismatchExt[t][a][b];
    }
    for (int x = tid; x < 40; x += nt) { T->dangle5[x / 5][x % 5] = P->dangle5[x / 5][x % 5]; T->dangle3[x / 5][x % 5] = P->dangle3[x / 5][x % 5]; }
    if (tid == 0) { T->ML_closing = P->ML_closing; T->ML_intern = P->ML_intern; T->TerminalAU = P->TerminalAU; T->ninio = P->ninio; T->MAX_NINIO = P->MAX_NINIO; }
    for (int x = tid; x < n; x += nt) S[x] = codes[x];
}

// the terms of oracle/lfold.c on the staged tables; a / b = -1: no neighbour
__device__ __forceinline__ int en_mlstem(const EnTables& T, int type, int a, int b) {
    int e = T.ML_intern + (type > 2 ? T.TerminalAU : 0);
    if (a >= 0 && b >= 0) e += T.mismatchM[type][a][b];
    else if (a >= 0) e += T.dangle5[type][a];
    else if (b >= 0) e += T.dangle3[type][b];
    return e;
}
__device__ __forceinline__ int en_extloop(const EnTables& T, int type, int a, int b) {
    int e = type > 2 ? T.TerminalAU : 0;
    if (a >= 0 && b >= 0) e += T.mismatchExt[type][a][b];
    else if (a >= 0) e += T.dangle5[type][a];
    else if (b >= 0) e += T.dangle3[type][b];
    return e;
}
// type2 already rtype'd; n1 + n2 <= 30; int11 / int21 / int22 from the resident FoldParams
__device__ __forceinline__ int en_intloop(const EnTables& T, const FoldParams* __restrict__ P, int n1, int n2, int type, int type2, int si1, int sj1, int sp1, int sq1) {
    const int nl = n1 > n2 ? n1 : n2, ns = n1 > n2 ? n2 : n1;
    if (nl == 0) return T.stack[type][type2];
    if (ns == 0) {
        int e = T.bulge[nl];
        if (nl == 1) e += T.stack[type][type2];
        else e += (type > 2 ? T.TerminalAU : 0) + (type2 > 2 ? T.TerminalAU : 0);
        return e;
    }
    if (ns == 1) {
        if (nl == 1) return P->int11[type][type2][si1][sj1];
        if (nl == 2) return n1 == 1 ? P->int21[type][type2][si1][sq1][sj1] : P->int21[type2][type][sq1][si1][sp1];
        const int x = (nl - 1) * T.ninio;
        return T.internal_loop[nl + 1] + (x < T.MAX_NINIO ? x : T.MAX_NINIO) + T.mismatch1nI[type][si1][sj1] + T.mismatch1nI[type2][sq1][sp1];
    }
    if (ns == 2) {
        if (nl == 2) return P->int22[type][type2][si1][sp1][sq1][sj1];
        if (nl == 3) return T.internal_loop[5] + T.ninio + T.mismatch23I[type][si1][sj1] + T.mismatch23I[type2][sq1][sp1];
    }
    const int x = (nl - ns) * T.ninio;
    return T.internal_loop[nl + ns] + (x < T.MAX_NINIO ? x : T.MAX_NINIO) + T.mismatchI[type][si1][sj1] + T.mismatchI[type2][sq1][sp1];
}

// hairpin closed by (i, j), 0-based; the motif tables hold letters, S holds codes N A C G U = 0..4
__device__ inline int en_hairpin(const EnTables& T, const FoldParams* __restrict__ P, const unsigned char* S, int i, int j, int type) {
    const int u = j - i - 1;
    if (u == 3 || u == 4 || u == 6) {
        const int n_mot = u == 3 ? P->n_tri : u == 4 ? P->n_tetra : P->n_hexa;
        for (int k = 0; k < n_mot; k++) {
            const char* mot = u == 3 ? P->tri[k] : u == 4 ? P->tetra[k] : P->hexa[k];
            bool same = true;
            for (int t = 0; t < u + 2; t++) same = same && mot[t] == "NACGU"[S[i + t]];
            if (same) return u == 3 ? P->triE[k] : u == 4 ? P->tetraE[k] : P->hexaE[k];
        }
        if (u == 3) return P->hairpinE[3] + (type > 2 ? T.TerminalAU : 0);
    }
    return P->hairpinE[u] + T.mismatchH[type][S[i + 1]][S[j - 1]];
}

}  // namespace
