// Stand-in for stb_image_write.h in the CPU build of the reference: WriteImage's JPEG is never written.
#pragma once
inline int stbi_write_jpg(const char *, int, int, int, const void *, int) { return 0; }
