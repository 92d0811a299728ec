// Body of count_gemm_reduce_kernel / _rows_kernel: included once per kernel, which sets IDX (and, where IDX is false, a null
// index pointer) in front of it -- see there.  Not a translation unit of its own.
  const size_t total = (size_t)M * N;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (size_t)gridDim.x * blockDim.x) {
    const int row = (int)(i / N), col = (int)(i % N);
    float s = 0.f;
    int z = 0;
    for (; z + 8 <= splits; z += 8) {      // (eight slabs' loads in flight, summed in slab order)
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = slabs[(size_t)(z + u) * total + i];
#pragma unroll
      for (int u = 0; u < 8; ++u) s += v[u];
    }
    for (; z < splits; ++z) s += slabs[(size_t)z * total + i];
    for (int k = k_main; k < K; ++k) {
      float xv;
      if constexpr (IDX) {   // (the cell -- the row of x -- through the resident matrix's row index)
        xv = count_to_f32(mode == 0 ? X[(size_t)xrows[row] * ldx + k] : X[(size_t)xrows[k] * ldx + row]);
      } else {
        xv = count_to_f32(mode == 0 ? X[(size_t)row * ldx + k] : X[(size_t)k * ldx + row]);
      }
      s = fmaf(xv, other[(size_t)k * ld_other + col], s);
    }
    if (bias) s += bias[col];
    if (act == ACT_RELU) s = relu_keep_nan(s);
    C[(size_t)row * ldc + col] = s;
  }
