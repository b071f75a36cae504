// Stand-in for stb_image.h in the CPU build of the reference: nothing on the render path decodes a file.
#pragma once
typedef unsigned char stbi_uc;
inline stbi_uc *stbi_load(const char *, int *x, int *y, int *comp, int) {
  *x = *y = *comp = 0;
  return nullptr;
}
inline void stbi_image_free(void *) {}
