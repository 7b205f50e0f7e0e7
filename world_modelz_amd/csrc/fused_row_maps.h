// The two row maps of a per-token launch on a compact grid (layer_fused.hip), stated once.  A launch works on B clips of rows_out
// rows each -- row t of the grid is row t % rows_out of clip t / rows_out -- and
//   reads  its input row (of x, or of the token grid z) at   fused_src_row: clip * rows_in  + row0     + row in clip
//          (the trailing-planes forms: a clip's input holds rows_in rows, the launch takes the last rows_out of them);
//   writes its q and k | v rows (the _slots forms only) at    fused_dst_row: clip * rows_dst + row0_dst + row in clip
//          (the context cache: a clip's q / k / v hold rows_dst rows -- whole plane slots --, the launch fills rows_out of them
//          from row0_dst on; the v rows start fused_dst_total rows behind the k rows).  x_out, and everything else, stays compact.
// rows_out == 0 is the identity (a launch that never asked for a map).  Plain integer code without HIP and without pointers:
// tests/context_cache_host.cpp runs these lines on the host, tests/test_context_cache_cpu.py says what they promise, the kernel's
// option policies (OptRuntime::src_row, OptSlots::dst_row) call them.
#pragma once
#ifdef __HIPCC__
#define WMZ_ROWMAP_FN __host__ __device__ __forceinline__
#else
#define WMZ_ROWMAP_FN inline
#endif

WMZ_ROWMAP_FN long fused_src_row(int rows_out, int rows_in, int row0, long t) {
  if (rows_out == 0) return t;
  const int c = (int)t / rows_out;
  return (long)c * rows_in + row0 + ((int)t - c * rows_out);
}

WMZ_ROWMAP_FN long fused_dst_row(int rows_out, int rows_dst, int row0_dst, long t) {
  if (rows_out == 0) return t;
  const int c = (int)t / rows_out;
  return (long)c * rows_dst + row0_dst + ((int)t - c * rows_out);
}

// rows of ONE of q, k, v in a launch's destination: B clips of rows_dst rows (where the v rows start behind the k rows)
WMZ_ROWMAP_FN long fused_dst_total(int B, int rows_dst) { return (long)B * rows_dst; }

// What the _slots entry points refuse: a launch writes the plane slots [dst_plane0, dst_plane0 + planes_out) of dst_planes
WMZ_ROWMAP_FN bool fused_slots_ok(int planes_out, int dst_planes, int dst_plane0) {
  return planes_out > 0 && dst_plane0 >= 0 && (long)dst_plane0 + planes_out <= dst_planes;
}
