// image_io.hpp -- the images bin/chan_vese reads and writes: binary PGM / PPM and PNG (png_io.hpp), the stand-ins for cv::imread /
// cv::imwrite (format by content on input, by extension on output), and the label image of --truth-labels.
#pragma once
#include <cctype>
#include <climits>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "png_io.hpp"

inline bool iequals(const std::string &a, const std::string &b)
{
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); ++i)
    if (std::tolower((unsigned char)a[i]) != std::tolower((unsigned char)b[i])) return false;
  return true;
}

// ---- PNM I/O ---------------------------------------------------------------------------
struct Image {
  int h = 0, w = 0, channels = 0;   // channels: 1 (P5) or 3 (P6, stored RGB interleaved)
  std::vector<uint8_t> px;
};

inline bool read_token(std::istream &in, std::string &tok)
{
  tok.clear();
  int c;
  while ((c = in.get()) != EOF) {
    if (c == '#') { while ((c = in.get()) != EOF && c != '\n') {} continue; }
    if (!std::isspace(c)) { tok.push_back((char)c); break; }
  }
  while ((c = in.peek()) != EOF && !std::isspace(c) && c != '#') tok.push_back((char)in.get());
  return !tok.empty();
}

// The header of a binary PNM whose magic is magic_a or magic_b and whose maxval lies in maxval_low .. maxval_top; leaves `in` at the samples.
inline bool read_pnm_header(std::istream &in, const char *magic_a, const char *magic_b, long maxval_low, long maxval_top, std::string &magic,
                            long &h, long &w, long &maxv)
{
  std::string sw, sh, smax;
  if (!read_token(in, magic) || (magic != magic_a && magic != magic_b)) return false;
  if (!read_token(in, sw) || !read_token(in, sh) || !read_token(in, smax)) return false;
  w = std::strtol(sw.c_str(), nullptr, 10); h = std::strtol(sh.c_str(), nullptr, 10);
  maxv = std::strtol(smax.c_str(), nullptr, 10);
  if (w <= 0 || h <= 0 || w > INT_MAX / 4 || h > INT_MAX / 4 || maxv < maxval_low || maxv > maxval_top) return false;
  in.get();  // the single whitespace after maxval
  return true;
}

inline bool read_pnm(const std::string &path, Image &img)
{
  std::ifstream in(path, std::ios::binary);
  if (!in) return false;
  std::string magic;
  long h, w, maxv;
  if (!read_pnm_header(in, "P5", "P6", 255, 255, magic, h, w, maxv)) return false;
  img.h = (int)h; img.w = (int)w; img.channels = magic == "P5" ? 1 : 3;
  img.px.resize((size_t)h * w * img.channels);
  in.read(reinterpret_cast<char *>(img.px.data()), (std::streamsize)img.px.size());
  return (size_t)in.gcount() == img.px.size();
}

// --truth-labels: a binary PGM with maxval <= 65535 (two bytes per sample, most significant first, above 255) or an 8-bit grey PNG; the
// values are the labels
inline bool read_labels(const std::string &path, int &h_out, int &w_out, std::vector<int32_t> &labels)
{
  if (pngio::is_png(path)) {
    pngio::Decoded d;
    const std::string err = pngio::read(path, d);
    if (!err.empty()) { std::cerr << "PNG: " << err << "\n"; return false; }
    if (d.channels != 1) return false;
    h_out = d.h; w_out = d.w;
    labels.assign(d.px.begin(), d.px.end());
    return true;
  }
  std::ifstream in(path, std::ios::binary);
  if (!in) return false;
  std::string magic;
  long h, w, maxv;
  if (!read_pnm_header(in, "P5", "P5", 1, 65535, magic, h, w, maxv)) return false;
  const size_t n = (size_t)h * w, width = maxv > 255 ? 2 : 1;
  std::vector<uint8_t> raw(n * width);
  in.read(reinterpret_cast<char *>(raw.data()), (std::streamsize)raw.size());
  if ((size_t)in.gcount() != raw.size()) return false;
  h_out = (int)h; w_out = (int)w;
  labels.resize(n);
  for (size_t q = 0; q < n; ++q) labels[q] = width == 2 ? (int32_t)raw[2 * q] << 8 | raw[2 * q + 1] : (int32_t)raw[q];
  return true;
}

inline bool write_pnm(const std::string &path, int h, int w, int channels, const uint8_t *px)
{
  std::ofstream out(path, std::ios::binary);
  if (!out) return false;
  out << (channels == 1 ? "P5" : "P6") << "\n" << w << " " << h << "\n255\n";
  out.write(reinterpret_cast<const char *>(px), (std::streamsize)((size_t)h * w * channels));
  return (bool)out;
}

// cv::imread / cv::imwrite stand-ins: format by content on input, by extension on output
inline bool has_ext(const std::string &path, const char *ext)
{
  const size_t n = std::strlen(ext);
  return path.size() >= n && iequals(path.substr(path.size() - n), ext);
}

inline bool read_image(const std::string &path, Image &img, bool &is_png)
{
  is_png = pngio::is_png(path);
  if (!is_png) return read_pnm(path, img);
  pngio::Decoded d;
  const std::string err = pngio::read(path, d);
  if (!err.empty()) { std::cerr << "PNG: " << err << "\n"; return false; }
  img.h = d.h; img.w = d.w; img.channels = d.channels; img.px.swap(d.px);
  return true;
}

inline bool write_image(const std::string &path, int h, int w, int channels, const uint8_t *px)
{
  if (has_ext(path, ".png")) return pngio::write(path, h, w, channels, px);
  return write_pnm(path, h, w, channels, px);
}
