// nexus/IMGLoader.h — image files to RGBA8 textures for the kept API surface.
// Mirrors /root/reference/Nexus/src/Assets/IMGLoader.h (IMGLoader::LoadIMG(path) / LoadIMG(embedded texture)), which wraps
// stb_image with 4 requested channels.  stb is an absent third-party dependency; this reader implements the PNG
// specification (ISO/IEC 15948) directly — zlib inflate, the five scanline filters, all colour types, 1-16 bit depth,
// palette and colour-key transparency — and yields what stbi_load(..., 4) yields: RGBA8, row 0 = top row, 16-bit samples
// reduced to their high byte.  Radiance .hdr files (RGBE, flat or run-length encoded: what the viewer's "Load HDR map" feeds
// through the same call, Renderer.cpp:104-117, Scene.cpp:93-97) are read too and reduced to 8 bits exactly as stbi_load
// does (gamma 2.2).  Not handled: Adam7 interlacing, JPEG files (an error message, never a crash).
#pragma once

#include <cstddef>
#include <string>

#include "Assets.h"

namespace nexus {

class IMGLoader {
public:
    // Throw std::runtime_error with a message on malformed / unsupported input.
    static Texture LoadIMG(const std::string& filepath);
    static Texture LoadIMG(const unsigned char* data, size_t size);
    // Extension: a Radiance .hdr file as what it holds — linear radiance, component = mantissa x 2^(e - 136), e = 0: 0 — instead of
    // the 8 bits LoadIMG reduces it to (pow(c, 1 / 2.2) x 255, clamped: a sun 10^5 times the sky comes out 50 times the sky).
    // The same RGBE reader (flat and run-length encoded scanlines), the same errors.
    static FloatImage LoadHDRFloat(const std::string& filepath);
    static FloatImage LoadHDRFloat(const unsigned char* data, size_t size);
    // Extension: a fog density grid from a NumPy .npy file (format version 1.x or 2.x) that holds little-endian float32 ('<f4') in C order
    // with the 3-D shape (nz, ny, nx) — what numpy.save writes for such an array.  Anything else (another dtype, Fortran order, another
    // rank, a truncated file) is refused with a message.  The values are not judged here: nxhip_set_medium_density validates them.
    static DensityGrid LoadNPYGrid(const std::string& filepath);
    static DensityGrid LoadNPYGrid(const unsigned char* data, size_t size);
};

}  // namespace nexus
