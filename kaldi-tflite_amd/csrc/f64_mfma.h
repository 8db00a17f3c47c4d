// The fp64 MFMA GEMM of this family (f64_mfma.hip): one kernel on v_mfma_f64_16x16x4_f64, instantiated for the two products below.
// Every output element is its starting value plus its terms in ascending k, four per MFMA, whatever M, N or the grid: the bits
// depend on the operands alone. All matrices fp64 row-major.
#pragma once
#include "common.h"

typedef double f64x4 __attribute__((ext_vector_type(4)));

// C (M x N, ldc) += A^T B: A (K x M, lda), B (K x N, ldb); the accumulators start from C
int f64_atb(const char* who, const double* A, int64_t lda, const double* Bm, int64_t ldb, double* Cm, int64_t ldc, int64_t M, int64_t N,
            int64_t K, hipStream_t st);

// C (M x N, ldc) = A B^T: A (M x K, lda), B (N x K, ldb); the accumulators start from zero
int f64_nt(const char* who, const double* A, int64_t lda, const double* Bm, int64_t ldb, double* Cm, int64_t ldc, int64_t M, int64_t N,
           int64_t K, hipStream_t st);
