// image.h — image file I/O of the host side (see image.cpp).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace mrt {

// Decode a scanline OpenEXR file into RGBA32F, row 0 = BOTTOM (the renderer's
// image orientation; loadReferenceImage flips the same way,
// renderer/Renderer.mm:233-235).  A missing A channel reads as 1.
bool load_exr(const std::string& path, std::vector<float>& rgba, uint32_t& width, uint32_t& height, std::string& err);

// Write an RGBA32F image (row 0 = bottom) as a PFM (RGB) or as an uncompressed
// scanline OpenEXR with FLOAT A, B, G, R channels.
bool write_pfm(const std::string& path, const std::vector<float>& rgba, uint32_t width, uint32_t height, std::string& err);
bool write_exr(const std::string& path, const std::vector<float>& rgba, uint32_t width, uint32_t height, std::string& err);

// The writer the path's extension names (.pfm / .exr).  On failure `io` tells a
// file that could not be written from an extension that names no writer.
bool save_rgba(const std::string& path, const std::vector<float>& rgba, uint32_t width, uint32_t height, std::string& err,
               bool& io);

}  // namespace mrt
