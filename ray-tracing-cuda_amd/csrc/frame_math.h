// Which pixel a work item is (rtmi_frame_pixel_of): one definition for every unit that asks.
#pragma once
// (included inside namespace rtmi, after scene_dev.h: FrameDev)

__host__ __device__ __forceinline__ int64_t frame_pixel_of_rank(const FrameDev &fr, int rank, int64_t q) {
  int64_t lt = q >> 6;
  int w = (int)(q & 63);
  int64_t gt = lt * fr.world + rank;
  if (gt >= fr.n_tiles) return -1;
  int ty = (int)(gt / fr.tiles_x), tx = (int)(gt % fr.tiles_x);
  int i = ty * 8 + (w >> 3), j = tx * 8 + (w & 7);
  if (i >= fr.height || j >= fr.width) return -1;
  return (int64_t)i * fr.width + j;
}
