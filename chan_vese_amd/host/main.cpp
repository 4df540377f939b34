// main.cpp — bin/chan_vese: the reference's command line over the MI355X HIP library.
//
// Keeps the CLI surface of the reference's main() (src/main.cpp:752-874: option names, short
// forms, defaults, multitoken --lambda1/--lambda2, validation order and messages, msg_exit
// behaviour, output naming through add_suffix) and its orchestration (:877-1007), but every
// array operation of the hot path goes through include/chanvese_hip.h into HIP kernels.
// No OpenCV/Boost: images are binary PGM/PPM or PNG (png_io.hpp over zlib), formats cv::imread
// also accepts; outputs keep the input's format like cv::imwrite by extension.
// Reference GUI code is out of scope: -R/--rectangle and -C/--circle (mouse selection) are parsed
// and validated as in the reference, then rejected with a message; their non-interactive forms are
// --rect x,y,w,h (1 inside / 0 outside, src/InteractiveDataRect.cpp:20-27) and --circ cx,cy,r
// (1-pixel outline of ones on zeros, src/InteractiveDataCirc.cpp:18-25).  Starts built on the device (chanvese_hip.h, "Device-side
// initial level sets"): --rect itself (cvh_init_rect), --disk cx,cy,r (a FILLED disk, 1 inside / 0 outside), --init otsu (+1 where the
// grey value exceeds Otsu's threshold, -1 elsewhere; with -S it is taken again from the smoothed planes) and --threshold T (the same
// with a given threshold); --init checkerboard is the default.
// -V/--video: the XVID writer (src/VideoWriterManager.cpp) is replaced by an image sequence
// <stem>_frames/frame_NNNNNN<ext> holding the same frames (the input with the contour drawn in
// --line-color, one frame for t = 0 and one after every iteration, :926-931,:997); the overlay
// text of -O is not rendered (no font rasteriser here), --fps has nothing to act on.
// --morph dilate|erode|open|close with --morph-radius R applies that operation by a disk to the cleaned mask on the device (chanvese_hip.h,
// "Mask morphology") for --dump-mask, --roi, --measure, --contours and _selection; --init-mask FILE starts from a binary PGM.
// Additions that do not collide with reference options: --dump-u, --dump-mask, --device, --math,
// --state, --rect, --circ, --disk, --init, --threshold, --reinit, --connectivity, --min-area, --fill-holes, --largest, --roi, --verbose,
// --levels, --energy, --energy-every, --truth, --score-tol, --measure, --contours, --contours-all, --contours-subpixel, --morph, --morph-radius, --init-mask, --truth-labels, --phases, --init2, --dump-labels, --localized (--localized R: cvh_localized_run, "Localised regions"; --phases 4: chanvese_hip.h, "Four phases" -- two contexts, cvh_multiphase_run, the labels; what does not compose with it is refused).  --truth-labels FILE
// relates the components of the mask --dump-mask uses (the cleaning options and -I apply) to the objects of a label image of the input's
// size (a binary PGM with maxval <= 65535 or an 8-bit grey PNG; the values are the labels, 0 = no object) on the device (chanvese_hip.h,
// "Component overlaps") and prints one line "objects: objects_a=... objects_b=... tp=... fp=... fn=... mean_ap=..." to stdout: the counts at
// IoU > 1/2, and the mean over 0.50 .. 0.95 of tp / (tp + fp + fn).  --contours FILE writes the boundary of
// the mask --dump-mask uses (the cleaning options and -I apply) as ordered closed loops traced on the device (chanvese_hip.h, "Contours"),
// one text line per loop: "first edges area2 :" and the x,y pairs of its corners, with --contours-all of every lattice vertex, with --contours-subpixel
// of the zero level's crossing of every edge (chanvese_hip.h, "Subpixel contours"; %.17g).  --measure FILE writes one CSV line per component of the mask --dump-mask
// uses (the cleaning options and -I apply), measured on the device (chanvese_hip.h, "Component measures"): label, the integers of the row,
// then centroid, central moments, orientation, axes, and mean and variance per channel (%.17g).  --truth FILE scores the final mask (inverted with -i) against a ground-truth PNG / PGM of
// the input's size (non-zero = foreground) on the device (chanvese_hip.h, "Mask scores") and prints one line "score: iou=... dice=...
// hausdorff=... assd=... surface_dice=... tp=... fp=... fn=... tn=..." to stdout; --score-tol T is the surface tolerance in pixels.  --energy prints "energy total length area fit_in... fit_out..." (chanvese_hip.h, "Energy"; %.17g, one
// fit_in and one fit_out per channel) to stdout after the run; --energy-every K runs in segments of K iterations and prints one such line,
// prefixed by the iteration count, after each (not with -V, --reinit, --levels).  --levels L > 1 is a coarse-to-fine run (chanvese_hip.h, "Coarse-to-fine"): L contexts, each half the one before; after -S
// the planes are restricted down the chain, the start is built on the COARSEST level (the numbers of --rect / --disk, given in pixels of
// the input, shifted right by L - 1; --init otsu / --threshold on the coarsest planes), and every level runs to its own stop (-N per
// level) before its level set is prolonged to the next.  Every level has the same parameters; nothing is rescaled.  --state 32 applies to
// the levels that qualify for it.  All outputs and the -V frames (the first one: the finest level's start) come from the finest level.
// --local mean|dev|stack with --local-radius R (chanvese_hip.h, "Local statistics"): the run iterates on the local mean / local deviation
// of every plane over the (2R+1)^2 window, or (stack, with -g) on the grey plane, its mean and its deviation as three planes, to which
// --lambda1 / --lambda2 with three values then apply; made on the device behind Perona-Malik and --colorspace, in front of the start, so
// --init otsu acts on the planes the run sees; --dump-planes FILE writes those planes.
// --rank median|min|max|open|close|tophat|bothat with --rank-radius R (chanvese_hip.h, "Rank planes"): the run iterates on that rank
// filter of every plane over the (2R+1)^2 window -- a median against impulse noise, a top-hat against a shading ramp; made on the device
// behind Perona-Malik and --colorspace, in front of --local (which then works on its result) and of the start; --dump-planes FILE writes
// the planes the run iterated on.
// --colorspace ycrcb|yuv (chanvese_hip.h, "Colour spaces"; not with -g): the loader's B, G, R planes become (Y, Cr, Cb) / (Y, U, V) on the
// device behind Perona-Malik -- <stem>_pm stays the RGB picture the reference writes -- and in front of the iterations (with --levels: on
// the finest level, before the restricts); --lambda1 / --lambda2 then weigh the luma and the two chroma planes, a start of --init otsu /
// --threshold is taken again from the converted planes, and nothing is converted back: frames, _selection and _contour use the input.
#include <algorithm>
#include <cctype>
#include <cerrno>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <limits>
#include <sstream>
#include <string>
#include <vector>

#include <sys/stat.h>

#include "chanvese_hip.h"
#include "png_io.hpp"
#include "overlay_text.hpp"

namespace {

// src/main.cpp:173-178
[[noreturn]] void msg_exit(const std::string &msg)
{
  std::cerr << "\n" << msg << "\n\n";
  std::exit(EXIT_FAILURE);
}

// src/main.cpp:158-167 (boost::filesystem parent_path / stem / extension semantics)
std::string add_suffix(const std::string &path, const std::string &suffix, const std::string &delim = "_")
{
  const size_t slash = path.find_last_of('/');
  const std::string parent = slash == std::string::npos ? "" : path.substr(0, slash);
  const std::string file = slash == std::string::npos ? path : path.substr(slash + 1);
  const size_t dot = file.find_last_of('.');
  const bool has_ext = dot != std::string::npos && dot != 0 && file != "..";
  const std::string stem = has_ext ? file.substr(0, dot) : file;
  const std::string ext = has_ext ? file.substr(dot) : "";
  const std::string name = stem + delim + suffix + ext;
  if (slash == std::string::npos) return name;
  return (parent.empty() ? std::string("/") : parent + "/") + name;
}

bool iequals(const std::string &a, const std::string &b)
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

bool read_token(std::istream &in, std::string &tok)
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

bool read_pnm(const std::string &path, Image &img)
{
  std::ifstream in(path, std::ios::binary);
  if (!in) return false;
  std::string magic, sw, sh, smax;
  if (!read_token(in, magic) || (magic != "P5" && magic != "P6")) return false;
  if (!read_token(in, sw) || !read_token(in, sh) || !read_token(in, smax)) return false;
  const long w = std::strtol(sw.c_str(), nullptr, 10), h = std::strtol(sh.c_str(), nullptr, 10);
  const long maxv = std::strtol(smax.c_str(), nullptr, 10);
  if (w <= 0 || h <= 0 || w > INT_MAX / 4 || h > INT_MAX / 4 || maxv != 255) return false;
  in.get();  // the single whitespace after maxval
  img.h = (int)h; img.w = (int)w; img.channels = magic == "P5" ? 1 : 3;
  img.px.resize((size_t)h * w * img.channels);
  in.read(reinterpret_cast<char *>(img.px.data()), (std::streamsize)img.px.size());
  return (size_t)in.gcount() == img.px.size();
}

// --truth-labels: a binary PGM with maxval <= 65535 (two bytes per sample, most significant first, above 255) or an 8-bit grey PNG; the
// values are the labels
bool read_labels(const std::string &path, int &h_out, int &w_out, std::vector<int32_t> &labels)
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
  std::string magic, sw, sh, smax;
  if (!read_token(in, magic) || magic != "P5") return false;
  if (!read_token(in, sw) || !read_token(in, sh) || !read_token(in, smax)) return false;
  const long w = std::strtol(sw.c_str(), nullptr, 10), h = std::strtol(sh.c_str(), nullptr, 10);
  const long maxv = std::strtol(smax.c_str(), nullptr, 10);
  if (w <= 0 || h <= 0 || w > INT_MAX / 4 || h > INT_MAX / 4 || maxv < 1 || maxv > 65535) return false;
  in.get();  // the single whitespace after maxval
  const size_t n = (size_t)h * w, width = maxv > 255 ? 2 : 1;
  std::vector<uint8_t> raw(n * width);
  in.read(reinterpret_cast<char *>(raw.data()), (std::streamsize)raw.size());
  if ((size_t)in.gcount() != raw.size()) return false;
  h_out = (int)h; w_out = (int)w;
  labels.resize(n);
  for (size_t q = 0; q < n; ++q) labels[q] = width == 2 ? (int32_t)raw[2 * q] << 8 | raw[2 * q + 1] : (int32_t)raw[q];
  return true;
}

bool write_pnm(const std::string &path, int h, int w, int channels, const uint8_t *px)
{
  std::ofstream out(path, std::ios::binary);
  if (!out) return false;
  out << (channels == 1 ? "P5" : "P6") << "\n" << w << " " << h << "\n255\n";
  out.write(reinterpret_cast<const char *>(px), (std::streamsize)((size_t)h * w * channels));
  return (bool)out;
}

// cv::imread / cv::imwrite stand-ins: format by content on input, by extension on output
bool has_ext(const std::string &path, const char *ext)
{
  const size_t n = std::strlen(ext);
  return path.size() >= n && iequals(path.substr(path.size() - n), ext);
}

bool read_image(const std::string &path, Image &img, bool &is_png)
{
  is_png = pngio::is_png(path);
  if (!is_png) return read_pnm(path, img);
  pngio::Decoded d;
  const std::string err = pngio::read(path, d);
  if (!err.empty()) { std::cerr << "PNG: " << err << "\n"; return false; }
  img.h = d.h; img.w = d.w; img.channels = d.channels; img.px.swap(d.px);
  return true;
}

bool write_image(const std::string &path, int h, int w, int channels, const uint8_t *px)
{
  if (has_ext(path, ".png")) return pngio::write(path, h, w, channels, px);
  return write_pnm(path, h, w, channels, px);
}

// cv::circle(u, centre, radius, 1) with the default thickness 1 and 8-connected line type
// (src/InteractiveDataCirc.cpp:24): OpenCV's integer midpoint circle, restated from memory of
// drawing.cpp (Circle): parity unpinned.
void draw_circle_outline(std::vector<double> &u, int h, int w, int cx, int cy, int radius)
{
  auto put = [&](int x, int y) { if (x >= 0 && x < w && y >= 0 && y < h) u[(size_t)y * w + x] = 1; };
  int err = 0, dx = radius, dy = 0, plus = 1, minus = (radius << 1) - 1;
  while (dx >= dy) {
    const int y11 = cy - dy, y12 = cy + dy, y21 = cy - dx, y22 = cy + dx;
    const int x11 = cx - dx, x12 = cx + dx, x21 = cx - dy, x22 = cx + dy;
    put(x11, y11); put(x12, y11); put(x11, y12); put(x12, y12);
    put(x21, y21); put(x22, y21); put(x21, y22); put(x22, y22);
    dy++;
    err += plus; plus += 2;
    const int mask = (err <= 0) - 1;
    err -= minus & mask;
    dx += mask;
    minus -= mask & 2;
  }
}

// ---- option parsing (the subset of boost::program_options behaviour the reference uses) --
struct Spec { const char *lname; char sname; int kind; };  // kind: 0 switch, 1 one value, 2 multitoken
const Spec kSpecs[] = {
    {"help", 'h', 0}, {"input", 'i', 1}, {"mu", 0, 1}, {"nu", 0, 1}, {"dt", 0, 1},
    {"lambda1", 0, 2}, {"lambda2", 0, 2}, {"epsilon", 'e', 1}, {"tolerance", 't', 1},
    {"max-steps", 'N', 1}, {"fps", 'f', 1}, {"overlay-pos", 'P', 1}, {"line-color", 'l', 1},
    {"edge-coef", 'K', 1}, {"laplacian-coef", 'L', 1}, {"segment-time", 'T', 1},
    {"segment", 'S', 0}, {"grayscale", 'g', 0}, {"video", 'V', 0}, {"overlay-text", 'O', 0},
    {"invert-selection", 'I', 0}, {"select", 's', 0}, {"rectangle", 'R', 0}, {"circle", 'C', 0},
    // additions of this build
    {"dump-u", 0, 1}, {"dump-mask", 0, 1}, {"device", 0, 1}, {"math", 0, 1}, {"state", 0, 1}, {"rect", 0, 1}, {"circ", 0, 1}, {"reinit", 0, 1},
    {"disk", 0, 1}, {"init", 0, 1}, {"threshold", 0, 1}, {"levels", 0, 1}, {"colorspace", 0, 1}, {"local", 0, 1}, {"local-radius", 0, 1}, {"dump-planes", 0, 1}, {"rank", 0, 1}, {"rank-radius", 0, 1},
    {"connectivity", 0, 1}, {"min-area", 0, 1}, {"fill-holes", 0, 1}, {"largest", 0, 0}, {"roi", 0, 0},
    {"verbose", 0, 0}, {"energy", 0, 0}, {"energy-every", 0, 1}, {"truth", 0, 1}, {"score-tol", 0, 1}, {"measure", 0, 1}, {"contours", 0, 1}, {"contours-all", 0, 0}, {"contours-subpixel", 0, 0},
    {"morph", 0, 1}, {"morph-radius", 0, 1}, {"init-mask", 0, 1}, {"truth-labels", 0, 1},
    {"phases", 0, 1}, {"init2", 0, 2}, {"dump-labels", 0, 1}, {"localized", 0, 1}};

struct Parsed {
  std::vector<std::pair<std::string, std::vector<std::string>>> opts;
  int count(const std::string &n) const { int c = 0; for (auto &o : opts) c += o.first == n; return c; }
  const std::vector<std::string> *get(const std::string &n) const
  {
    const std::vector<std::string> *r = nullptr;
    for (auto &o : opts) if (o.first == n) r = &o.second;
    return r;
  }
};

const Spec *find_long(const std::string &n)
{
  const Spec *hit = nullptr;
  int hits = 0;
  for (const Spec &s : kSpecs) {
    if (n == s.lname) return &s;
    if (std::string(s.lname).compare(0, n.size(), n) == 0) { hit = &s; ++hits; }  // unambiguous prefix
  }
  return hits == 1 ? hit : nullptr;
}
const Spec *find_short(char c)
{
  for (const Spec &s : kSpecs) if (s.sname && s.sname == c) return &s;
  return nullptr;
}
bool looks_like_option(const std::string &t) { return t.size() >= 2 && t[0] == '-' && !std::isdigit((unsigned char)t[1]) && t[1] != '.'; }

Parsed parse_args(int argc, char **argv)
{
  Parsed p;
  for (int i = 1; i < argc; ++i) {
    std::string tok = argv[i];
    const Spec *sp = nullptr;
    std::string attached;
    bool has_attached = false;
    if (tok.rfind("--", 0) == 0) {
      std::string name = tok.substr(2);
      const size_t eq = name.find('=');
      if (eq != std::string::npos) { attached = name.substr(eq + 1); name = name.substr(0, eq); has_attached = true; }
      sp = find_long(name);
      if (!sp) msg_exit("error: unrecognised option '" + tok.substr(0, eq == std::string::npos ? std::string::npos : eq + 2) + "'");
    } else if (tok.size() >= 2 && tok[0] == '-') {
      sp = find_short(tok[1]);
      if (!sp) msg_exit("error: unrecognised option '" + tok.substr(0, 2) + "'");
      if (tok.size() > 2) {
        if (sp->kind == 0) {  // grouped switches: -gs
          for (size_t k = 1; k < tok.size(); ++k) {
            const Spec *s2 = find_short(tok[k]);
            if (!s2 || s2->kind != 0) msg_exit(std::string("error: unrecognised option '-") + tok[k] + "'");
            p.opts.push_back({s2->lname, {}});
          }
          continue;
        }
        attached = tok.substr(2); has_attached = true;
      }
    } else {
      msg_exit("error: too many positional options have been specified on the command line");
    }
    std::vector<std::string> vals;
    if (sp->kind == 0) {
      if (has_attached) msg_exit(std::string("error: option '--") + sp->lname + "' does not take any arguments");
    } else if (sp->kind == 1) {
      if (has_attached) vals.push_back(attached);
      else if (i + 1 < argc && !looks_like_option(argv[i + 1])) vals.push_back(argv[++i]);
      else msg_exit(std::string("error: the required argument for option '--") + sp->lname + "' is missing");
    } else {
      if (has_attached) vals.push_back(attached);
      while (i + 1 < argc && !looks_like_option(argv[i + 1])) vals.push_back(argv[++i]);
      if (vals.empty()) msg_exit(std::string("error: the required argument for option '--") + sp->lname + "' is missing");
    }
    if (sp->kind != 2 && p.count(sp->lname) > 0 && sp->kind == 1)
      msg_exit(std::string("error: option '--") + sp->lname + "' cannot be specified more than once");
    p.opts.push_back({sp->lname, vals});
  }
  return p;
}

double to_double(const std::string &opt, const std::string &v)
{
  char *end = nullptr;
  const double d = std::strtod(v.c_str(), &end);
  if (v.empty() || *end != '\0') msg_exit("error: the argument ('" + v + "') for option '--" + opt + "' is invalid");
  return d;
}
long to_long(const std::string &opt, const std::string &v)
{
  char *end = nullptr;
  errno = 0;
  const long d = std::strtol(v.c_str(), &end, 10);
  if (v.empty() || *end != '\0' || errno == ERANGE) msg_exit("error: the argument ('" + v + "') for option '--" + opt + "' is invalid");
  return d;
}
int to_int(const std::string &opt, const std::string &v)
{
  char *end = nullptr;
  const long d = std::strtol(v.c_str(), &end, 10);
  if (v.empty() || *end != '\0' || d > INT_MAX || d < INT_MIN) msg_exit("error: the argument ('" + v + "') for option '--" + opt + "' is invalid");
  return (int)d;
}

// --local and --rank: a windowed filter by name, which stands for the code of every plane, and the radius of its window
// (--local-radius, --rank-radius), which one name (`bound`) may bind to less than radius_max
struct WindowName { const char *name; int code; };   // (a table ends with a null name)
struct WindowOption { const char *key, *label, *noun; const WindowName *names; int radius_max; const char *bound; int bound_max; };
const WindowName kLocalNames[] = {{"mean", CVH_LOCAL_MEAN}, {"dev", CVH_LOCAL_DEV}, {"stack", CVH_LOCAL_COPY}, {nullptr, 0}};   // (stack: main)
const WindowName kRankNames[] = {{"median", CVH_RANK_MEDIAN}, {"min", CVH_RANK_MIN}, {"max", CVH_RANK_MAX}, {"open", CVH_RANK_OPEN},
                                 {"close", CVH_RANK_CLOSE}, {"tophat", CVH_RANK_TOPHAT}, {"bothat", CVH_RANK_BOTHAT}, {nullptr, 0}};
const WindowOption kLocalOption = {"local", "Local", "statistic", kLocalNames, CVH_LOCAL_RADIUS_MAX, "", 0};
const WindowOption kRankOption = {"rank", "Rank", "filter", kRankNames, CVH_RANK_RADIUS_MAX, "median", CVH_RANK_MEDIAN_RADIUS_MAX};

// Whether the option is given; then every what[k] receives the code of `name` and `radius` is checked against the name's range.
// Refuses an unknown name and a radius without a name.
bool window_option(const Parsed &vm, const WindowOption &o, const std::string &name, int radius, int what[3])
{
  const std::string key = o.key;
  if (!vm.count(key)) {
    if (vm.count(key + "-radius")) msg_exit("A radius (--" + key + "-radius) needs a " + o.noun + " (--" + key + ").");
    return false;
  }
  const WindowName *hit = nullptr;
  std::string list;
  for (const WindowName *nm = o.names; nm->name; ++nm) {
    if (iequals(name, nm->name)) hit = nm;
    list += std::string(list.empty() ? "" : ", ") + nm->name;
  }
  if (!hit) msg_exit("Invalid " + key + " " + o.noun + " requested.\nCorrect values are: " + list + ".");
  const bool bound = iequals(name, o.bound);
  const int top = bound ? o.bound_max : o.radius_max;
  if (radius < 0 || radius > top)
    msg_exit(std::string(o.label) + " radius must be between 0 and " + std::to_string(top) + (bound ? " for a " + std::string(o.bound) : "") + ": " + std::to_string(radius) + ".");
  what[0] = what[1] = what[2] = hit->code;
  return true;
}

void print_help()
{
  std::cout <<
      "Allowed options:\n"
      "  -h [ --help ]                      this message\n"
      "  -i [ --input ] arg                 input image (binary PGM/PPM)\n"
      "  --mu arg (=0.5)                    length penalty parameter (must be positive or zero)\n"
      "  --nu arg (=0)                      area penalty parameter\n"
      "  --dt arg (=1)                      timestep\n"
      "  --lambda1 arg                      penalty of variance inside the contour (default: 1's)\n"
      "  --lambda2 arg                      penalty of variance outside the contour (default: 1's)\n"
      "  -e [ --epsilon ] arg (=1)          smoothing parameter in Heaviside/delta\n"
      "  -t [ --tolerance ] arg (=0.001)    tolerance in stopping condition\n"
      "  -N [ --max-steps ] arg (=-1)       maximum nof iterations (negative means unlimited)\n"
      "  -f [ --fps ] arg (=10)             video fps\n"
      "  -P [ --overlay-pos ] arg (=TL)     overlay tex position; allowed only: TL, BL, TR, BR\n"
      "  -l [ --line-color ] arg (=blue)    contour color (allowed only: black, white, R, G, B, Y, M, C\n"
      "  -K [ --edge-coef ] arg (=10)       coefficient for enhancing edge detection in Perona-Malik\n"
      "  -L [ --laplacian-coef ] arg (=0.25) coefficient in the gradient FD scheme of Perona-Malik (must be [0, 1/4])\n"
      "  -T [ --segment-time ] arg (=20)    number of smoothing steps in Perona-Malik\n"
      "  -S [ --segment ]                   segment the image with Perona-Malik beforehand\n"
      "  -g [ --grayscale ]                 read in as grayscale\n"
      "  -V [ --video ]                     enable video output (here: image sequence <stem>_frames/frame_NNNNNN<ext>)\n"
      "  -O [ --overlay-text ]              add overlay text\n"
      "  -I [ --invert-selection ]          invert selected region (see: select)\n"
      "  -s [ --select ]                    separate the region encolosed by the contour (adds suffix '_selection')\n"
      "  -R [ --rectangle ]                 select rectangular contour interactively (not supported in this build)\n"
      "  -C [ --circle ]                    select circular contour interactively (not supported in this build)\n"
      "MI355X build additions:\n"
      "  --rect x,y,w,h                     rectangular initial contour (1 inside, 0 outside)\n"
      "  --circ cx,cy,r                     circular initial contour (1-pixel outline of ones on zeros)\n"
      "  --disk cx,cy,r                     filled disk as initial contour, built on the device (1 inside, 0 outside)\n"
      "  --init arg (=checkerboard)         checkerboard | otsu: otsu starts from Otsu's threshold of the grey values (the sum of the\n"
      "                                     channels), +1 above it and -1 elsewhere, built on the device (with -S: of the smoothed image)\n"
      "  --threshold T                      the same start with the threshold T (0 .. 255 x channels) instead of Otsu's\n"
      "  --dump-u arg                       write the final level set as raw little-endian float64 (h*w)\n"
      "  --dump-mask arg                    write the final mask ((float)u > 0) as PGM or PNG by extension (0/255)\n"
      "  --device arg (=0)                  HIP device\n"
      "  --math arg (=fast)                 strict | fast (see include/chanvese_hip.h)\n"
      "  --state arg (=64)                  64 | 32: level set kept as double (the reference's CV_64FC1) or, DECLARED, as float in GPU memory\n"
      "  --reinit arg (=0)                  reinitialise the level set to a signed distance every arg iterations (0: never); -N stays the total\n"
      "  --connectivity arg (=4)            4 | 8: connectivity of the mask's components (the background takes the other one)\n"
      "  --min-area arg (=0)                drop components of the mask with fewer pixels\n"
      "  --fill-holes arg (=0)              fill holes of the mask up to arg pixels (-1: of any size)\n"
      "  --largest                          keep only the largest component of the mask\n"
      "                                     (with any of these four, _selection and --dump-mask use the cleaned mask)\n"
      "  --roi                              print 'roi x0 y0 x1 y1 area' of that mask's largest component to stdout\n"
      "  --levels arg (=1)                  coarse-to-fine run over arg levels, each half the one before: the start is built and iterated\n"
      "                                     on the coarsest level, then handed up level by level (-N counts per level); not with --circ, --reinit\n"
      "  --local arg                        mean | dev | stack: iterate on the local mean / local deviation of every plane, or (with -g) on\n"
      "                                     the grey plane, its local mean and its local deviation as three planes; made on the device behind\n"
      "                                     Perona-Malik and --colorspace, in front of the initial level set\n"
      "  --local-radius arg (=2)            radius R of the (2R+1) x (2R+1) window of --local, 0 .. 127\n"
      "  --rank arg                         median | min | max | open | close | tophat | bothat: iterate on that rank filter of every plane;\n"
      "                                     made on the device behind Perona-Malik and --colorspace, in front of --local and the initial level set\n"
      "  --rank-radius arg (=1)             radius R of the (2R+1) x (2R+1) window of --rank, 0 .. 127 (median: 0 .. 7)\n"
      "  --dump-planes arg                  write the planes the run iterated on, one under the other, as PGM or PNG by extension\n"
      "  --colorspace arg                   ycrcb | yuv: iterate on (Y, Cr, Cb) / (Y, U, V) planes, converted on the device behind Perona-Malik\n"
      "                                     (--lambda1 / --lambda2 then weigh Y, the first and the second chroma plane: 0 1 1 ignores shading;\n"
      "                                     --init otsu / --threshold act on the converted planes); not with -g\n"
      "  --energy                           print 'energy total length area fit_in... fit_out...' of the final level set to stdout (%.17g)\n"
      "  --energy-every arg (=0)            run in segments of arg iterations and print such a line, prefixed by the iteration count, after\n"
      "                                     each (0: never); -N stays the total; not with -V, --reinit, --levels\n"
      "  --truth arg                        ground-truth PNG / PGM of the input's size (non-zero = foreground): print 'score: iou= dice=\n"
      "                                     hausdorff= assd= surface_dice= tp= fp= fn= tn=' of the final mask (inverted with -i) to stdout\n"
      "  --truth-labels arg                 label image of the input's size (binary PGM, maxval <= 65535, or 8-bit grey PNG; 0 = no object):\n"
      "                                     print 'objects: objects_a= objects_b= tp= fp= fn= mean_ap=' for the components of the mask (the\n"
      "                                     cleaning options and -I apply) against its objects at IoU > 1/2, mean_ap over 0.50 .. 0.95\n"
      "  --score-tol arg (=2)               surface tolerance of --truth in pixels (surface_dice counts distances <= arg)\n"
      "  --measure arg                      write one CSV line per component of the mask --dump-mask uses (cleaning options, -I): label,\n"
      "                                     first,area,x0,y0,x1,y1,border,perimeter,cx,cy,mu20,mu02,mu11,theta,major,minor,mean..,var..\n"
      "  --contours arg                     write the boundary of the mask --dump-mask uses (cleaning options, -I) as closed loops, one\n"
      "                                     line per loop: 'first edges area2 :' and the x,y pairs of its corners in order\n"
      "  --contours-all                     --contours keeps every lattice vertex, not the corners alone\n"
      "  --contours-subpixel                --contours writes the zero level of the level set instead: one x,y pair (%.17g) per edge of\n"
      "                                     the loop, where the level set changes sign across it\n"
      "  --morph arg                        dilate | erode | open | close: that operation by a disk of --morph-radius pixels, on the device,\n"
      "                                     behind the cleaning options: --dump-mask, --roi, --measure, --contours and _selection use its result\n"
      "  --morph-radius arg (=1)            radius R of that disk in pixels: the offsets with dx^2 + dy^2 <= floor(R^2) (1: the 4-neighbour cross)\n"
      "  --phases arg (=2)                  2 | 4: four phases evolve TWO level sets together (Vese-Chan), whose sign pairs name four classes;\n"
      "                                     -s then writes the label plane as a grey image (label x 85); not with -V, --levels, --energy,\n"
      "                                     --energy-every, --reinit (nor the mask-based outputs, which take one level set)\n"
      "  --init2 arg (=checkerboard)        checkerboard | otsu | threshold T: the start of the second level set (--phases 4); the\n"
      "                                     checkerboard is --init's rolled by (2, 3) pixels\n"
      "  --dump-labels arg                  write the labels (mask 1 + 2 mask 2, one byte per pixel, h*w) of a --phases 4 run\n"
      "  --localized arg                    R, 1 .. 127: localised Chan-Vese -- the two region means are taken over the (2R+1)^2 window of every\n"
      "                                     pixel and retaken every iteration (uneven illumination); honours --init, --rect, --circ, --disk and\n"
      "                                     --init-mask; start near the object and raise --mu (of the order of 100); not with --phases 4,\n"
      "                                     --levels, --energy, --energy-every, --reinit, -V\n"
      "  --init-mask arg                    binary PGM of the input's size as the initial contour (+1 where it is non-zero, -1 elsewhere),\n"
      "                                     written on the device at a byte per pixel; not with --levels\n"
      "  --verbose                          print the iteration count and last norm to stderr\n"
      "\n";
}

void cvh_check(cvh_context *ctx, int rc, const char *what)
{
  if (rc != CVH_OK) msg_exit(std::string("Error: ") + what + ": " + cvh_last_error(ctx));
}

}  // namespace

int main(int argc, char **argv)
{
  // defaults: src/main.cpp:759-772
  double mu = 0.5, nu = 0, eps = 1, tol = 0.001, dt = 1, fps = 10, K = 10, L = 0.25, T = 20;
  int max_steps = -1, device = 0;
  std::vector<double> lambda1, lambda2;
  std::string input_filename, text_position = "TL", line_color_str = "blue", dump_u, dump_mask, math = "fast", rect, circ;
  bool grayscale = false, write_video = false, overlay_text = false, object_selection = false, invert = false,
       segment = false, rectangle_contour = false, circle_contour = false;

  const Parsed vm = parse_args(argc, argv);
  auto one = [&](const char *n) -> const std::string * { auto v = vm.get(n); return v && !v->empty() ? &(*v)[0] : nullptr; };
  if (auto v = one("input")) input_filename = *v;
  if (auto v = one("mu")) mu = to_double("mu", *v);
  if (auto v = one("nu")) nu = to_double("nu", *v);
  if (auto v = one("dt")) dt = to_double("dt", *v);
  if (auto v = vm.get("lambda1")) for (auto &s : *v) lambda1.push_back(to_double("lambda1", s));
  if (auto v = vm.get("lambda2")) for (auto &s : *v) lambda2.push_back(to_double("lambda2", s));
  if (auto v = one("epsilon")) eps = to_double("epsilon", *v);
  if (auto v = one("tolerance")) tol = to_double("tolerance", *v);
  if (auto v = one("max-steps")) max_steps = to_int("max-steps", *v);
  if (auto v = one("fps")) fps = to_double("fps", *v);
  if (auto v = one("overlay-pos")) text_position = *v;
  if (auto v = one("line-color")) line_color_str = *v;
  if (auto v = one("edge-coef")) K = to_double("edge-coef", *v);
  if (auto v = one("laplacian-coef")) L = to_double("laplacian-coef", *v);
  if (auto v = one("segment-time")) T = to_double("segment-time", *v);
  if (auto v = one("dump-u")) dump_u = *v;
  if (auto v = one("dump-mask")) dump_mask = *v;
  if (auto v = one("device")) device = to_int("device", *v);
  if (auto v = one("math")) math = *v;
  int state_bits = 64;
  if (auto v = one("state")) state_bits = to_int("state", *v);
  int reinit_every = 0;
  if (auto v = one("reinit")) reinit_every = to_int("reinit", *v);
  int connectivity = 4;
  long min_area = 0, fill_holes = 0;
  if (auto v = one("connectivity")) connectivity = to_int("connectivity", *v);
  if (auto v = one("min-area")) min_area = to_long("min-area", *v);
  if (auto v = one("fill-holes")) fill_holes = to_long("fill-holes", *v);
  bool largest = vm.count("largest");
  const bool roi = vm.count("roi");
  bool clean_mask = vm.count("connectivity") || vm.count("min-area") || vm.count("fill-holes") || largest;
  std::string morph_name, init_mask_filename;
  double morph_radius = 1.0;
  if (auto v = one("morph")) morph_name = *v;
  if (auto v = one("morph-radius")) morph_radius = to_double("morph-radius", *v);
  if (auto v = one("init-mask")) init_mask_filename = *v;
  if (auto v = one("rect")) rect = *v;
  if (auto v = one("circ")) circ = *v;
  std::string disk, init_kind = "checkerboard";
  int threshold = -1;
  if (auto v = one("disk")) disk = *v;
  if (auto v = one("init")) init_kind = *v;
  if (auto v = one("threshold")) threshold = to_int("threshold", *v);
  int levels = 1;
  if (auto v = one("levels")) levels = to_int("levels", *v);
  std::string colorspace;
  if (auto v = one("colorspace")) colorspace = *v;
  std::string local_name, dump_planes;
  if (auto v = one("local")) local_name = *v;
  if (auto v = one("dump-planes")) dump_planes = *v;
  std::string rank_name;
  if (auto v = one("rank")) rank_name = *v;
  int rank_radius = 1;
  if (auto v = one("rank-radius")) rank_radius = to_int("rank-radius", *v);
  int local_radius = 2;
  if (auto v = one("local-radius")) local_radius = to_int("local-radius", *v);
  const bool print_energy = vm.count("energy");
  int energy_every = 0;
  if (auto v = one("energy-every")) energy_every = to_int("energy-every", *v);
  std::string truth_filename;
  if (auto v = one("truth")) truth_filename = *v;
  std::string truth_labels_filename;
  if (auto v = one("truth-labels")) truth_labels_filename = *v;
  std::string measure_filename;
  if (auto v = one("measure")) measure_filename = *v;
  std::string contours_filename;
  if (auto v = one("contours")) contours_filename = *v;
  const bool contours_all = vm.count("contours-all") > 0;
  const bool contours_subpixel = vm.count("contours-subpixel") > 0;
  double score_tol = 2.0;
  if (auto v = one("score-tol")) score_tol = to_double("score-tol", *v);
  int phases = 2;
  if (auto v = one("phases")) phases = to_int("phases", *v);
  std::string dump_labels;
  if (auto v = one("dump-labels")) dump_labels = *v;
  int localized = 0;   // --localized R (chanvese_hip.h, "Localised regions"): cvh_localized_run in place of cvh_run
  if (auto v = one("localized")) {
    localized = to_int("localized", *v);
    if (localized < 1 || localized > 127) msg_exit("Window radius (--localized) must be between 1 and 127: " + std::to_string(localized) + ".");
  }
  segment = vm.count("segment"); grayscale = vm.count("grayscale"); write_video = vm.count("video");
  overlay_text = vm.count("overlay-text"); invert = vm.count("invert-selection");
  object_selection = vm.count("select"); rectangle_contour = vm.count("rectangle"); circle_contour = vm.count("circle");
  (void)fps;

  // ---- validation, in the reference's order with its messages: src/main.cpp:786-869
  if (vm.count("help")) { print_help(); return EXIT_SUCCESS; }
  if (!vm.count("input")) msg_exit("Error: you have to specify input file name!");
  else if (!std::ifstream(input_filename).good()) msg_exit("Error: file \"" + input_filename + "\" does not exists!");
  if (dt <= 0) msg_exit("Cannot have negative or zero timestep: " + std::to_string(dt) + ".");
  if (mu < 0) msg_exit("Length penalty parameter cannot be negative: " + std::to_string(mu) + ".");
  // --local: the run iterates on local statistics of the planes (chanvese_hip.h, "Local statistics"); stack turns the grey plane into three
  int local_what[3] = {CVH_LOCAL_COPY, CVH_LOCAL_COPY, CVH_LOCAL_COPY};
  const bool local_stack = vm.count("local") > 0 && iequals(local_name, "stack");
  if (local_stack && !grayscale) msg_exit("The local stack (--local stack) needs a grayscale read (-g): it makes three planes of one.");
  const bool local = window_option(vm, kLocalOption, local_name, local_radius, local_what);
  if (local_stack) { local_what[1] = CVH_LOCAL_MEAN; local_what[2] = CVH_LOCAL_DEV; }
  // --rank: the run iterates on a rank filter of the planes (chanvese_hip.h, "Rank planes"), every plane alike
  int rank_what[3] = {CVH_RANK_COPY, CVH_RANK_COPY, CVH_RANK_COPY};
  const bool rank = window_option(vm, kRankOption, rank_name, rank_radius, rank_what);
  const bool one_plane = grayscale && !local_stack;   // the run has one plane: what the lambda counts and the threshold range follow
  if (vm.count("lambda1")) {
    if (one_plane && lambda1.size() != 1) msg_exit("Too many lambda1 values for a grayscale image.");
    else if (!one_plane && lambda1.size() != 3) msg_exit("Number of lambda1 values must be 3 for a colored input image.");
    else if (one_plane && lambda1[0] < 0) msg_exit("The value of lambda1 cannot be negative.");
    else if (!one_plane && (lambda1[0] < 0 || lambda1[1] < 0 || lambda1[2] < 0)) msg_exit("Any value of lambda1 cannot be negative.");
  } else {
    lambda1 = one_plane ? std::vector<double>{1} : std::vector<double>{1, 1, 1};
  }
  if (vm.count("lambda2")) {
    if (one_plane && lambda2.size() != 1) msg_exit("Too many lambda2 values for a grayscale image.");
    else if (!one_plane && lambda2.size() != 3) msg_exit("Number of lambda2 values must be 3 for a colored input image.");
    else if (one_plane && lambda2[0] < 0) msg_exit("The value of lambda2 cannot be negative.");
    else if (!one_plane && (lambda2[0] < 0 || lambda2[1] < 0 || lambda2[2] < 0)) msg_exit("Any value of lambda2 cannot be negative.");
  } else {
    lambda2 = one_plane ? std::vector<double>{1} : std::vector<double>{1, 1, 1};
  }
  // (the reference's eps/tol checks look up non-existent keys and never fire: src/main.cpp:831-834)
  if (!(iequals(text_position, "TL") || iequals(text_position, "BL") || iequals(text_position, "TR") || iequals(text_position, "BR")))
    msg_exit("Invalid text position requested.\nCorrect values are: TL -- top left\n"
             "                    BL -- bottom left\n                    TR -- top right\n"
             "                    BR -- bottom right");
  {
    const char *colors[] = {"red", "green", "blue", "black", "white", "magenta", "yellow", "cyan"};
    bool ok = false;
    for (const char *c : colors) ok = ok || iequals(line_color_str, c);
    if (!ok) msg_exit("Invalid contour color requested.\nCorrect values are: red, green, blue, black, white, magenta, yellow, cyan.");
  }
  if (L > 0.25 || L < 0) msg_exit("The Laplacian coefficient in Perona-Malik segmentation must be between 0 and 0.25.");
  if (vm.count("segment-time") && T < L)
    msg_exit("The segmentation duration must exceed the value of Laplacian coefficient, " + std::to_string(L) + ".");
  if (rectangle_contour && circle_contour) msg_exit("Cannot initialize with both rectangular and circular contour");
  if (rectangle_contour || circle_contour)
    msg_exit("Interactive contour selection (-R/-C) needs a display and is not supported in this build; use --rect x,y,w,h or --circ cx,cy,r.");
  if (!rect.empty() && !circ.empty()) msg_exit("Cannot initialize with both rectangular and circular contour");
  if (init_kind != "checkerboard" && init_kind != "otsu") msg_exit("error: the argument ('" + init_kind + "') for option '--init' is invalid");
  const bool init_otsu = init_kind == "otsu", init_threshold = vm.count("threshold") > 0;
  {
    std::vector<std::string> given;
    if (!rect.empty()) given.push_back("--rect");
    if (!circ.empty()) given.push_back("--circ");
    if (!disk.empty()) given.push_back("--disk");
    if (init_otsu) given.push_back("--init otsu");
    if (init_threshold) given.push_back("--threshold");
    if (!init_mask_filename.empty()) given.push_back("--init-mask");
    if (given.size() > 1) msg_exit("Cannot initialize with both " + given[0] + " and " + given[1]);
  }
  int disk_cx = 0, disk_cy = 0, disk_r = 0;
  if (!disk.empty()) {
    char rest = 0;
    if (std::sscanf(disk.c_str(), "%d,%d,%d%c", &disk_cx, &disk_cy, &disk_r, &rest) != 3 || disk_r < 0)
      msg_exit("You must specify the disk as cx,cy,r with a radius that is not negative");
  }
  if (init_threshold && (threshold < 0 || threshold > 255 * (one_plane ? 1 : 3)))
    msg_exit("Threshold must be between 0 and " + std::to_string(255 * (one_plane ? 1 : 3)) + ": " + std::to_string(threshold) + ".");
  if (math != "strict" && math != "fast") msg_exit("error: the argument ('" + math + "') for option '--math' is invalid");
  if (state_bits != 64 && state_bits != 32) msg_exit("error: the argument ('" + std::to_string(state_bits) + "') for option '--state' is invalid");
  if (reinit_every < 0) msg_exit("Reinitialisation interval cannot be negative: " + std::to_string(reinit_every) + ".");
  if (connectivity != 4 && connectivity != 8) msg_exit("Connectivity must be 4 or 8: " + std::to_string(connectivity) + ".");
  if (min_area < 0) msg_exit("Minimum component area cannot be negative: " + std::to_string(min_area) + ".");
  if (fill_holes < -1) msg_exit("Largest hole to fill must be -1 (any size), zero or positive: " + std::to_string(fill_holes) + ".");
  if (reinit_every > 0 && write_video) msg_exit("Reinitialisation (--reinit) cannot be combined with video output (-V).");
  if (levels < 1) msg_exit("Number of levels must be at least 1: " + std::to_string(levels) + ".");
  if (levels > 1 && reinit_every > 0) msg_exit("Reinitialisation (--reinit) cannot be combined with a coarse-to-fine run (--levels).");
  if (levels > 1 && !circ.empty()) msg_exit("A circular outline (--circ) cannot be combined with a coarse-to-fine run (--levels); use --disk.");
  if (energy_every < 0) msg_exit("Energy interval cannot be negative: " + std::to_string(energy_every) + ".");
  if (!contours_filename.empty() && write_video) msg_exit("A contour file (--contours) cannot be combined with video output (-V).");
  if (contours_all && contours_filename.empty()) msg_exit("Every lattice vertex (--contours-all) needs a contour file (--contours).");
  if (contours_subpixel && contours_filename.empty()) msg_exit("Subpixel points (--contours-subpixel) need a contour file (--contours).");
  if (contours_subpixel && contours_all) msg_exit("Subpixel points (--contours-subpixel) cannot be combined with every lattice vertex (--contours-all).");
  if (energy_every > 0 && write_video) msg_exit("An energy series (--energy-every) cannot be combined with video output (-V).");
  if (energy_every > 0 && reinit_every > 0) msg_exit("An energy series (--energy-every) cannot be combined with reinitialisation (--reinit).");
  if (energy_every > 0 && levels > 1) msg_exit("An energy series (--energy-every) cannot be combined with a coarse-to-fine run (--levels).");
  // --phases 4 (chanvese_hip.h, "Four phases"): two level sets, the second one started by --init2; what does not compose with it is refused
  if (phases != 2 && phases != 4) msg_exit("Number of phases must be 2 or 4: " + std::to_string(phases) + ".");
  std::string init2_kind = "checkerboard";
  int threshold2 = -1;
  if (auto v = vm.get("init2")) {
    if (phases != 4) msg_exit("A second start (--init2) needs four phases (--phases 4).");
    if (v->empty()) msg_exit("error: the required argument for option '--init2' is missing");
    init2_kind = (*v)[0];
    if (init2_kind == "threshold") {
      if (v->size() != 2) msg_exit("A threshold start (--init2 threshold T) needs its threshold.");
      threshold2 = to_int("init2", (*v)[1]);
      if (threshold2 < 0 || threshold2 > 255 * (one_plane ? 1 : 3))
        msg_exit("Threshold must be between 0 and " + std::to_string(255 * (one_plane ? 1 : 3)) + ": " + std::to_string(threshold2) + ".");
    } else if ((init2_kind != "checkerboard" && init2_kind != "otsu") || v->size() != 1) {
      msg_exit("error: the argument ('" + init2_kind + "') for option '--init2' is invalid");
    }
  }
  if (!dump_labels.empty() && phases != 4) msg_exit("A label file (--dump-labels) needs four phases (--phases 4).");
  if (phases == 4) {
    const std::pair<bool, const char *> refused[] = {
        {write_video, "video output (-V)"}, {levels > 1, "a coarse-to-fine run (--levels)"}, {print_energy, "an energy line (--energy)"},
        {energy_every > 0, "an energy series (--energy-every)"}, {reinit_every > 0, "reinitialisation (--reinit)"},
        // the rest of what this build does not carry through two level sets: nothing is silently ignored
        {state_bits == 32, "FP32 state (--state 32)"}, {!rect.empty(), "--rect"}, {!circ.empty(), "--circ"}, {!disk.empty(), "--disk"},
        {!init_mask_filename.empty(), "--init-mask"}, {vm.count("local") > 0, "--local"}, {vm.count("rank") > 0, "--rank"},
        {vm.count("colorspace") > 0, "--colorspace"}, {!dump_planes.empty(), "--dump-planes"}, {!dump_u.empty(), "--dump-u"},
        {!dump_mask.empty(), "--dump-mask"}, {clean_mask, "the cleaning options"}, {roi, "--roi"}, {vm.count("morph") > 0, "--morph"},
        {!truth_filename.empty(), "--truth"}, {!truth_labels_filename.empty(), "--truth-labels"}, {!measure_filename.empty(), "--measure"},
        {!contours_filename.empty(), "--contours"}, {invert, "an inverted selection (-I)"}};
    for (auto &r : refused)
      if (r.first) msg_exit(std::string("Four phases (--phases 4) cannot be combined with ") + r.second + ".");
  }
  if (localized) {
    const std::pair<bool, const char *> refused[] = {
        {phases == 4, "four phases (--phases 4)"}, {levels > 1, "a coarse-to-fine run (--levels)"}, {print_energy, "an energy line (--energy)"},
        {energy_every > 0, "an energy series (--energy-every)"}, {reinit_every > 0, "reinitialisation (--reinit)"},
        {write_video, "video output (-V)"}, {state_bits == 32, "FP32 state (--state 32)"}};
    for (auto &r : refused)
      if (r.first) msg_exit(std::string("Localised regions (--localized) cannot be combined with ") + r.second + ".");
  }
  if (vm.count("score-tol") && truth_filename.empty()) msg_exit("A score tolerance (--score-tol) needs a ground truth (--truth).");
  if (!(score_tol >= 0.0) || !std::isfinite(score_tol)) msg_exit("Score tolerance must be a finite number >= 0.");
  int morph_op = CVH_MORPH_NONE;
  if (vm.count("morph")) {
    if (morph_name == "dilate") morph_op = CVH_MORPH_DILATE;
    else if (morph_name == "erode") morph_op = CVH_MORPH_ERODE;
    else if (morph_name == "open") morph_op = CVH_MORPH_OPEN;
    else if (morph_name == "close") morph_op = CVH_MORPH_CLOSE;
    else msg_exit("Invalid morphology requested.\nCorrect values are: dilate, erode, open, close.");
  }
  if (vm.count("morph-radius") && !vm.count("morph")) msg_exit("A radius (--morph-radius) needs an operation (--morph).");
  if (!(morph_radius >= 0.0) || !std::isfinite(morph_radius)) msg_exit("Morphology radius must be a finite number >= 0.");
  const double morph_r2d = std::floor(morph_radius * morph_radius);
  const uint32_t morph_r2 = morph_r2d >= 4294967295.0 ? 0xffffffffu : (uint32_t)morph_r2d;
  if (!init_mask_filename.empty() && levels > 1)
    msg_exit("A mask start (--init-mask) cannot be combined with a coarse-to-fine run (--levels): a mask is not resampled.");
  if (!init_mask_filename.empty() && !std::ifstream(init_mask_filename).good())
    msg_exit("Error: file \"" + init_mask_filename + "\" does not exists!");
  int colour_space = 0;   // 0: the planes stay B, G, R
  if (vm.count("colorspace")) {
    if (iequals(colorspace, "ycrcb")) colour_space = CVH_COLOUR_YCRCB;
    else if (iequals(colorspace, "yuv")) colour_space = CVH_COLOUR_YUV;
    else msg_exit("Invalid colour space requested.\nCorrect values are: ycrcb, yuv.");
    if (grayscale) msg_exit("A colour space (--colorspace) cannot be combined with a grayscale read (-g): there is one plane.");
  }

  // ---- read the image: src/main.cpp:877-887 (8-bit gray or BGR)
  Image file;
  bool input_is_png = false;
  if (!read_image(input_filename, file, input_is_png)) msg_exit("Error on opening \"" + input_filename + "\" (probably not an image)!");
  if (!input_is_png && has_ext(input_filename, ".png")) msg_exit("Error on opening \"" + input_filename + "\" (probably not an image)!");
  const int h = file.h, w = file.w;
  const size_t n = (size_t)h * w;
  const int nof_channels = grayscale ? 1 : 3;          // planes read from the file
  const int run_channels = one_plane ? 1 : 3;           // planes the run iterates on (--local stack: three of one)
  std::vector<uint8_t> truth;   // --truth: one byte per pixel, non-zero = foreground
  if (!truth_filename.empty()) {
    Image t;
    bool truth_is_png = false;
    if (!read_image(truth_filename, t, truth_is_png)) msg_exit("Error on opening \"" + truth_filename + "\" (probably not an image)!");
    if (t.h != h || t.w != w)
      msg_exit("The ground truth \"" + truth_filename + "\" is " + std::to_string(t.w) + " x " + std::to_string(t.h) + ", the input " +
               std::to_string(w) + " x " + std::to_string(h) + ": they must have the same size.");
    truth.resize(n);
    for (size_t q = 0; q < n; ++q) {
      uint8_t any = 0;
      for (int k = 0; k < t.channels; ++k) any |= t.px[(size_t)t.channels * q + k];
      truth[q] = any;
    }
  }
  std::vector<int32_t> truth_labels;   // --truth-labels: one label per pixel
  if (!truth_labels_filename.empty()) {
    int th = 0, tw = 0;
    if (!read_labels(truth_labels_filename, th, tw, truth_labels))
      msg_exit("Error on opening \"" + truth_labels_filename + "\" (a label image must be a binary PGM with maxval <= 65535 or an 8-bit grey PNG)!");
    if (th != h || tw != w)
      msg_exit("The label image \"" + truth_labels_filename + "\" is " + std::to_string(tw) + " x " + std::to_string(th) + ", the input " +
               std::to_string(w) + " x " + std::to_string(h) + ": they must have the same size.");
  }
  std::vector<uint8_t> init_mask;   // --init-mask: one byte per pixel, non-zero = inside
  if (!init_mask_filename.empty()) {
    Image t;
    if (!read_pnm(init_mask_filename, t) || t.channels != 1)
      msg_exit("Error on opening \"" + init_mask_filename + "\" (a mask start must be a binary PGM)!");
    if (t.h != h || t.w != w)
      msg_exit("The mask start \"" + init_mask_filename + "\" is " + std::to_string(t.w) + " x " + std::to_string(t.h) + ", the input " +
               std::to_string(w) + " x " + std::to_string(h) + ": they must have the same size.");
    init_mask.assign(t.px.begin(), t.px.begin() + (std::ptrdiff_t)n);
  }
  // img: what the reference calls `img` (3 channels, BGR); planes: what cv::split leaves (:934-937)
  std::vector<uint8_t> img_bgr(n * 3);
  std::vector<std::vector<uint8_t>> planes(nof_channels, std::vector<uint8_t>(n));
  for (size_t q = 0; q < n; ++q) {
    uint8_t b, g, r;
    if (file.channels == 1) { b = g = r = file.px[q]; }
    else { r = file.px[3 * q]; g = file.px[3 * q + 1]; b = file.px[3 * q + 2]; }
    if (grayscale) {
      // cv::imread(..., GRAYSCALE) of a colour file.  PxM decoder: icvCvt_BGR2Gray_8u_C3C1R, 14-bit fixed
      // point BT.601 (R 4899, G 9617, B 1868).  PNG decoder: libpng's png_set_rgb_to_gray(0.299, 0.587),
      // 15-bit fixed point (R 9798, G 19235, B 3735, rounded; equal channels pass through).
      uint8_t y;
      if (file.channels == 1) y = b;
      else if (!input_is_png) y = (uint8_t)((r * 4899 + g * 9617 + b * 1868 + 8192) >> 14);
      else y = (r == g && g == b) ? r : (uint8_t)((r * 9798 + g * 19235 + b * 3735 + 16384) >> 15);
      img_bgr[3 * q] = img_bgr[3 * q + 1] = img_bgr[3 * q + 2] = y;  // cvtColor GRAY2RGB (:885)
      planes[0][q] = y;
    } else {
      img_bgr[3 * q] = b; img_bgr[3 * q + 1] = g; img_bgr[3 * q + 2] = r;
      planes[0][q] = b; planes[1][q] = g; planes[2][q] = r;
    }
  }

  // ---- constants: src/main.cpp:890-895
  max_steps = max_steps < 0 ? std::numeric_limits<int>::max() : max_steps;
  cvh_params prm;
  cvh_default_params(&prm);
  prm.mu = mu; prm.nu = nu; prm.dt = dt; prm.eps = eps; prm.tol = tol;
  for (int k = 0; k < run_channels; ++k) { prm.lambda1[k] = lambda1[k]; prm.lambda2[k] = lambda2[k]; }

  // ---- four phases: two contexts hold phi1 and phi2 and the same planes; everything of this run is here
  if (phases == 4) {
    cvh_context *pa = nullptr, *pb = nullptr;
    for (cvh_context **c : {&pa, &pb}) {
      if (cvh_create(c, h, w, run_channels, &prm, device) != CVH_OK)
        msg_exit(std::string("Error: cannot initialise the HIP backend: ") + cvh_last_error(nullptr));
      cvh_check(*c, cvh_set_option(*c, "math_mode", math == "strict" ? CVH_MATH_STRICT : CVH_MATH_FAST), "math_mode");
    }
    std::vector<uint8_t *> pp;
    for (auto &p : planes) pp.push_back(p.data());
    cvh_check(pa, cvh_set_image(pa, pp.data()), "cvh_set_image");
    if (segment) {   // src/main.cpp:940-947, once: B takes the smoothed bytes
      cvh_check(pa, cvh_perona_malik(pa, K, L, T), "cvh_perona_malik");
      cvh_check(pa, cvh_get_image(pa, pp.data()), "cvh_get_image");
      std::vector<uint8_t> out(n * nof_channels);
      for (size_t q = 0; q < n; ++q) {
        if (nof_channels == 1) out[q] = planes[0][q];
        else { out[3 * q] = planes[2][q]; out[3 * q + 1] = planes[1][q]; out[3 * q + 2] = planes[0][q]; }
      }
      if (!write_image(add_suffix(input_filename, "pm"), h, w, nof_channels, out.data()))
        msg_exit("Error: cannot write \"" + add_suffix(input_filename, "pm") + "\"");
    }
    cvh_check(pb, cvh_set_image(pb, pp.data()), "cvh_set_image");
    if (init_otsu) cvh_check(pa, cvh_init_otsu(pa, nullptr, 1.0, -1.0), "cvh_init_otsu");
    else if (init_threshold) cvh_check(pa, cvh_init_threshold(pa, threshold, 1.0, -1.0), "cvh_init_threshold");
    else cvh_check(pa, cvh_init_checkerboard(pa), "cvh_init_checkerboard");
    if (init2_kind == "otsu") cvh_check(pb, cvh_init_otsu(pb, nullptr, 1.0, -1.0), "cvh_init_otsu");
    else if (init2_kind == "threshold") cvh_check(pb, cvh_init_threshold(pb, threshold2, 1.0, -1.0), "cvh_init_threshold");
    else {   // the checkerboard rolled by (2, 3) pixels: two identical starts would stay identical forever
      std::vector<double> cb(n), u2(n);
      cvh_levelset_checkerboard_host(h, w, cb.data());
      for (int i = 0; i < h; ++i)
        for (int j = 0; j < w; ++j) u2[(size_t)((i + 2) % h) * w + (size_t)((j + 3) % w)] = cb[(size_t)i * w + j];
      cvh_check(pb, cvh_set_levelset(pb, u2.data()), "cvh_set_levelset");
    }
    int steps4 = 0;
    double norms4[2] = {0, 0};
    if (cvh_multiphase_run(pa, pb, max_steps, &steps4, norms4, nullptr, 0, nullptr) != CVH_OK)
      msg_exit(std::string("Error: cvh_multiphase_run: ") + cvh_last_error(nullptr));
    std::vector<uint8_t> labels(n);
    if (cvh_multiphase_labels(pa, pb, labels.data()) != CVH_OK)
      msg_exit(std::string("Error: cvh_multiphase_labels: ") + cvh_last_error(nullptr));
    if (!dump_labels.empty()) {
      std::ofstream out(dump_labels, std::ios::binary);
      out.write(reinterpret_cast<const char *>(labels.data()), (std::streamsize)n);
      if (!out) msg_exit("Error: cannot write \"" + dump_labels + "\"");
    }
    if (object_selection) {   // the label plane as a grey image: label x 85
      std::vector<uint8_t> grey(n);
      for (size_t q = 0; q < n; ++q) grey[q] = (uint8_t)(labels[q] * 85);
      if (!write_image(add_suffix(input_filename, "selection"), h, w, 1, grey.data()))
        msg_exit("Error: cannot write \"" + add_suffix(input_filename, "selection") + "\"");
    }
    if (vm.count("verbose"))
      std::fprintf(stderr, "four phases: %d iterations, norms %.17g %.17g\n", steps4, norms4[0], norms4[1]);
    cvh_destroy(pb);
    cvh_destroy(pa);
    return EXIT_SUCCESS;
  }

  std::vector<std::pair<int, int>> level_shape{{h, w}};   // finest first
  for (int k = 1; k < levels; ++k) level_shape.push_back({(level_shape.back().first + 1) / 2, (level_shape.back().second + 1) / 2});
  if (std::min(level_shape.back().first, level_shape.back().second) < 16 && levels > 1)
    msg_exit("Too many levels for a " + std::to_string(h) + " x " + std::to_string(w) + " image: the coarsest side must not fall below 16.");

  cvh_context *ctx = nullptr;
  if (cvh_create(&ctx, h, w, run_channels, &prm, device) != CVH_OK)
    msg_exit(std::string("Error: cannot initialise the HIP backend: ") + cvh_last_error(nullptr));
  cvh_check(ctx, cvh_set_option(ctx, "math_mode", math == "strict" ? CVH_MATH_STRICT : CVH_MATH_FAST), "math_mode");
  if (state_bits == 32) cvh_check(ctx, cvh_set_option(ctx, "state", 32), "state");   // declared FP32-state mode: never the default
  std::vector<cvh_context *> level{ctx};   // the helper levels of a coarse-to-fine run: idle while another level runs ("co_resident")
  for (int k = 1; k < levels; ++k) {
    cvh_context *c = nullptr;
    if (cvh_create(&c, level_shape[k].first, level_shape[k].second, run_channels, &prm, device) != CVH_OK)
      msg_exit(std::string("Error: cannot initialise the HIP backend: ") + cvh_last_error(nullptr));
    cvh_check(c, cvh_set_option(c, "math_mode", math == "strict" ? CVH_MATH_STRICT : CVH_MATH_FAST), "math_mode");
    if (state_bits == 32) (void)cvh_set_option(c, "state", 32);   // (a level too narrow for it keeps 64)
    cvh_check(c, cvh_set_option(c, "co_resident", 0), "co_resident");
    level.push_back(c);
  }
  cvh_context *const coarsest = level.back();
  const int shift = levels - 1;
  // --local: the file's planes go into a context of their own, where they are smoothed and converted; ctx, the one that runs, receives
  // their local statistics -- here, for a start taken from the image and the t = 0 frame, and again behind -S and --colorspace
  // --rank goes the same way and in front of --local: with both, the rank planes land in a context of their own that --local reads
  cvh_context *ingest = ctx, *ranked = ctx;
  if (local || rank) {
    if (cvh_create(&ingest, h, w, nof_channels, nullptr, device) != CVH_OK)
      msg_exit(std::string("Error: cannot initialise the HIP backend: ") + cvh_last_error(nullptr));
    cvh_check(ingest, cvh_set_option(ingest, "co_resident", 0), "co_resident");
  }
  if (local && rank) {
    if (cvh_create(&ranked, h, w, nof_channels, nullptr, device) != CVH_OK)
      msg_exit(std::string("Error: cannot initialise the HIP backend: ") + cvh_last_error(nullptr));
    cvh_check(ranked, cvh_set_option(ranked, "co_resident", 0), "co_resident");
  }
  auto local_planes = [&]() {
    if (rank) cvh_check(ranked, cvh_rank_planes(ingest, ranked, rank_radius, rank_what), "cvh_rank_planes");
    if (local) cvh_check(ctx, cvh_local_planes(rank ? ranked : ingest, ctx, local_radius, local_what), "cvh_local_planes");
  };
  {
    std::vector<const uint8_t *> pp;
    for (auto &p : planes) pp.push_back(p.data());
    cvh_check(ingest, cvh_set_image(ingest, pp.data()), "cvh_set_image");
    local_planes();
  }

  // ---- level set: src/main.cpp:898-923.  A coarse-to-fine run builds it on the coarsest level, from planes that are restricted only
  // after Perona-Malik: not here but through the same lambda below
  int rx = 0, ry = 0, rw = 0, rh = 0;
  if (!rect.empty() && (std::sscanf(rect.c_str(), "%d,%d,%d,%d", &rx, &ry, &rw, &rh) != 4 || rw <= 0 || rh <= 0))
    msg_exit("You must specify the contour with non-zero dimensions");
  auto device_start = [&](cvh_context *c, int sh) {   // the starts built on the device, their numbers shifted right by sh
    if (!rect.empty()) cvh_check(c, cvh_init_rect(c, rx >> sh, ry >> sh, rw >> sh, rh >> sh, 1.0, 0.0), "cvh_init_rect");   // src/InteractiveDataRect.cpp:24-25
    else if (!disk.empty()) cvh_check(c, cvh_init_disk(c, disk_cx >> sh, disk_cy >> sh, disk_r >> sh, 1.0, 0.0), "cvh_init_disk");
    else if (init_otsu) cvh_check(c, cvh_init_otsu(c, nullptr, 1.0, -1.0), "cvh_init_otsu");
    else if (init_threshold) cvh_check(c, cvh_init_threshold(c, threshold, 1.0, -1.0), "cvh_init_threshold");
    else cvh_check(c, cvh_init_checkerboard(c), "cvh_init_checkerboard");
  };
  if (levels > 1) {
  } else if (!rect.empty() || !disk.empty() || init_otsu || init_threshold) {
    device_start(ctx, 0);
  } else if (!init_mask.empty()) {
    cvh_check(ctx, cvh_init_mask(ctx, init_mask.data(), 1.0, -1.0), "cvh_init_mask");
  } else if (!circ.empty()) {
    int cx, cy, cr;
    if (std::sscanf(circ.c_str(), "%d,%d,%d", &cx, &cy, &cr) != 3 || cr <= 0)  // is_ok(): radius > 0
      msg_exit("You must specify the contour with non-zero dimensions");
    std::vector<double> u(n, 0.0);  // src/InteractiveDataCirc.cpp:23-24
    draw_circle_outline(u, h, w, cx, cy, cr);
    cvh_check(ctx, cvh_set_levelset(ctx, u.data()), "cvh_set_levelset");
  } else {
    cvh_check(ctx, cvh_init_checkerboard(ctx), "cvh_init_checkerboard");
  }

  // ---- video frames: src/main.cpp:926-931 (first frame before the channels are split / smoothed)
  const size_t dot = input_filename.find_last_of('.');
  const size_t slash = input_filename.find_last_of('/');
  const bool with_ext = dot != std::string::npos && (slash == std::string::npos || dot > slash + 1);
  const std::string frames_dir = (with_ext ? input_filename.substr(0, dot) : input_filename) + "_frames";
  const std::string frame_ext = with_ext ? input_filename.substr(dot) : std::string(".ppm");
  uint8_t contour_bgr[3] = {255, 0, 0};  // ChanVese::Colors::blue = CV_RGB(0,0,255), src/main.cpp:111-118,747
  {
    struct { const char *name; uint8_t r, g, b; } table[] = {{"red", 255, 0, 0}, {"green", 0, 255, 0}, {"blue", 0, 0, 255},
      {"black", 0, 0, 0}, {"white", 255, 255, 255}, {"magenta", 255, 0, 255}, {"yellow", 255, 255, 0}, {"cyan", 0, 255, 255}};
    for (auto &e : table) if (iequals(line_color_str, e.name)) { contour_bgr[0] = e.b; contour_bgr[1] = e.g; contour_bgr[2] = e.r; }
  }
  int frame_no = 0;
  std::vector<uint8_t> contour, frame;
  overlay::Pos opos = overlay::Pos::TL;   // src/main.cpp:837-849
  if (iequals(text_position, "BL")) opos = overlay::Pos::BL;
  else if (iequals(text_position, "TR")) opos = overlay::Pos::TR;
  else if (iequals(text_position, "BR")) opos = overlay::Pos::BR;
  auto write_frame = [&](const std::string &txt) {  // VideoWriterManager::write_frame, src/VideoWriterManager.cpp:40-57
    contour.resize(n); frame.resize(n * 3);
    cvh_check(ctx, cvh_get_contour(ctx, contour.data()), "cvh_get_contour");
    for (size_t q = 0; q < n; ++q) {   // frames are RGB files; img_bgr is the reference's `img`
      const bool c = contour[q] != 0;
      frame[3 * q] = c ? contour_bgr[2] : img_bgr[3 * q + 2];
      frame[3 * q + 1] = c ? contour_bgr[1] : img_bgr[3 * q + 1];
      frame[3 * q + 2] = c ? contour_bgr[0] : img_bgr[3 * q];
    }
    if (overlay_text && !txt.empty()) {   // :47-53: colour and corner from overlay_color (:76-114), own 5x7 glyphs
      int px, py; bool black;
      overlay::place(img_bgr.data(), h, w, txt, opos, &px, &py, &black);
      overlay::draw(frame.data(), h, w, txt, px, py, black);
    }
    char name[64];
    std::snprintf(name, sizeof(name), "/frame_%06d", frame_no++);
    const std::string path = frames_dir + name + (has_ext(frame_ext, ".png") ? ".png" : ".ppm");
    if (!write_image(path, h, w, 3, frame.data())) msg_exit("Error: cannot write \"" + path + "\"");
  };
  if (write_video) {
    if (mkdir(frames_dir.c_str(), 0777) != 0 && errno != EEXIST) msg_exit("Error: cannot create \"" + frames_dir + "\"");
    if (levels == 1) write_frame("t = 0");   // :930
  }

  // ---- Perona-Malik: src/main.cpp:940-947
  if (segment) {
    cvh_check(ingest, cvh_perona_malik(ingest, K, L, T), "cvh_perona_malik");
    std::vector<uint8_t *> pp;
    for (auto &p : planes) pp.push_back(p.data());
    cvh_check(ingest, cvh_get_image(ingest, pp.data()), "cvh_get_image");
    local_planes();
    std::vector<uint8_t> out(n * nof_channels);
    for (size_t q = 0; q < n; ++q) {
      if (nof_channels == 1) out[q] = planes[0][q];
      else { out[3 * q] = planes[2][q]; out[3 * q + 1] = planes[1][q]; out[3 * q + 2] = planes[0][q]; }  // BGR -> RGB file order
    }
    if (!write_image(add_suffix(input_filename, "pm"), h, w, nof_channels, out.data()))
      msg_exit("Error: cannot write \"" + add_suffix(input_filename, "pm") + "\"");
    // a start taken from the image is taken again from the smoothed planes (the one above served the t = 0 frame)
    if (levels > 1) {}
    else if (init_otsu) cvh_check(ctx, cvh_init_otsu(ctx, nullptr, 1.0, -1.0), "cvh_init_otsu");
    else if (init_threshold) cvh_check(ctx, cvh_init_threshold(ctx, threshold, 1.0, -1.0), "cvh_init_threshold");
  }

  // ---- colour space: behind Perona-Malik (<stem>_pm stays the picture the reference writes), in front of the iterations.  The loader's
  // planes are B, G, R.  Nothing is converted back: frames, _selection and _contour use the input image.  A start taken from the image
  // is taken again from the converted planes, as behind -S
  if (colour_space) {
    cvh_check(ingest, cvh_convert_colour(ingest, colour_space, CVH_ORDER_BGR, 0), "cvh_convert_colour");
    local_planes();
    if (levels > 1) {}
    else if (init_otsu) cvh_check(ctx, cvh_init_otsu(ctx, nullptr, 1.0, -1.0), "cvh_init_otsu");
    else if (init_threshold) cvh_check(ctx, cvh_init_threshold(ctx, threshold, 1.0, -1.0), "cvh_init_threshold");
  }

  // ---- timestep loop: src/main.cpp:950-1001 (stop condition and every iteration on the GPU)
  int steps_done = 0;
  double last_norm = 0;
  std::vector<int> level_steps((size_t)levels, 0);
  auto run_with_frames = [&]() {   // one iteration per frame; the frame is saved before the stop test (:997-1000)
    for (int t = 1; t <= max_steps; ++t) {
      int stopped = 0;
      cvh_check(ctx, cvh_enqueue_steps(ctx, 1), "cvh_enqueue_steps");
      cvh_check(ctx, cvh_sync(ctx, &steps_done, &last_norm, &stopped), "cvh_sync");
      write_frame("t = " + std::to_string(t));   // :997
      if (stopped) break;
    }
  };
  auto energy_line = [&](int iteration) {   // "[iteration ]energy total length area fit_in... fit_out...", every number %.17g
    cvh_energy_terms e;
    cvh_check(ctx, cvh_energy(ctx, &e), "cvh_energy");
    if (iteration >= 0) std::printf("%d ", iteration);
    std::printf("energy %.17g %.17g %.17g", e.total, e.length, e.area);
    for (int k = 0; k < run_channels; ++k) std::printf(" %.17g", e.fit_in[k]);
    for (int k = 0; k < run_channels; ++k) std::printf(" %.17g", e.fit_out[k]);
    std::printf("\n");
    std::fflush(stdout);
  };
  if (levels > 1) {
    // restrict down the chain, start on the coarsest level, then level by level: run, prolong.  While a level runs the others do not
    // count in its automatic choices ("co_resident"); the finest keeps its own value throughout
    for (int k = 0; k + 1 < levels; ++k) cvh_check(level[k + 1], cvh_restrict_image(level[k], level[k + 1]), "cvh_restrict_image");
    device_start(coarsest, shift);
    for (int k = levels - 1; k >= 0; --k) {
      if (k + 1 < levels) cvh_check(level[k], cvh_prolong_levelset(level[k + 1], level[k]), "cvh_prolong_levelset");
      if (k > 0) {
        cvh_check(level[k], cvh_set_option(level[k], "co_resident", 1), "co_resident");
        cvh_check(level[k], cvh_run(level[k], max_steps, &level_steps[k], nullptr), "cvh_run");
        cvh_check(level[k], cvh_set_option(level[k], "co_resident", 0), "co_resident");
      } else if (!write_video) {
        cvh_check(ctx, cvh_run(ctx, max_steps, &steps_done, &last_norm), "cvh_run");
      } else {
        write_frame("t = 0");
        run_with_frames();
      }
    }
    level_steps[0] = steps_done;
  } else if (reinit_every > 0) {
    // segments of reinit_every iterations, the level set re-distanced between them; a stop inside a segment ends the run
    for (int left = max_steps; left > 0;) {
      const int k = std::min(reinit_every, left);
      int done = 0, stopped = 0;
      cvh_check(ctx, cvh_run(ctx, k, &done, &last_norm), "cvh_run");
      cvh_check(ctx, cvh_sync(ctx, nullptr, nullptr, &stopped), "cvh_sync");
      steps_done += done;
      left -= k;
      if (stopped) break;
      if (left > 0) cvh_check(ctx, cvh_reinit(ctx, nullptr), "cvh_reinit");
    }
  } else if (energy_every > 0) {
    // segments of energy_every iterations, the energy taken behind each; a stop inside a segment ends the run
    for (int left = max_steps; left > 0;) {
      const int k = std::min(energy_every, left);
      int done = 0, stopped = 0;
      cvh_check(ctx, cvh_run(ctx, k, &done, &last_norm), "cvh_run");
      cvh_check(ctx, cvh_sync(ctx, nullptr, nullptr, &stopped), "cvh_sync");
      steps_done += done;
      left -= k;
      energy_line(steps_done);
      if (stopped) break;
    }
  } else if (localized) {
    cvh_check(ctx, cvh_localized_run(ctx, localized, max_steps, &steps_done, &last_norm, nullptr, 0, nullptr), "cvh_localized_run");
  } else if (!write_video) {
    cvh_check(ctx, cvh_run(ctx, max_steps, &steps_done, &last_norm), "cvh_run");
  } else {
    run_with_frames();
  }
  if (print_energy) energy_line(-1);
  if (!truth.empty()) {   // the derived figures as the header spells them; nan where a denominator is 0 or a surface is empty
    cvh_mask_score s;
    const double t2 = std::floor(score_tol * score_tol);
    cvh_check(ctx, cvh_score_mask(ctx, truth.data(), invert ? 1 : 0, t2 >= 4294967295.0 ? 0xffffffffu : (uint32_t)t2, &s), "cvh_score_mask");
    const double nan = std::numeric_limits<double>::quiet_NaN();
    auto ratio = [&](double num, double den) { return den != 0.0 ? num / den : nan; };
    const double surf = (double)(s.surf_m + s.surf_t);
    std::printf("score: iou=%.17g dice=%.17g hausdorff=%.17g assd=%.17g surface_dice=%.17g tp=%llu fp=%llu fn=%llu tn=%llu\n",
                ratio((double)s.tp, (double)(s.tp + s.fp + s.fn)), ratio(2.0 * (double)s.tp, (double)(2 * s.tp + s.fp + s.fn)),
                s.defined ? std::sqrt((double)std::max(s.hd2_m, s.hd2_t)) : nan,
                s.defined ? ratio((double)(s.dist_m_q16 + s.dist_t_q16) / 65536.0, surf) : nan,
                s.defined ? ratio((double)(s.within_m + s.within_t), surf) : nan, (unsigned long long)s.tp, (unsigned long long)s.fp,
                (unsigned long long)s.fn, (unsigned long long)s.tn);
  }

  if (!dump_planes.empty()) {   // the planes the run iterated on, one under the other
    std::vector<uint8_t> all(n * run_channels);
    std::vector<uint8_t *> pp;
    for (int k = 0; k < run_channels; ++k) pp.push_back(all.data() + (size_t)k * n);
    cvh_check(ctx, cvh_get_image(ctx, pp.data()), "cvh_get_image");
    if (!write_image(dump_planes, h * run_channels, w, 1, all.data())) msg_exit("Error: cannot write \"" + dump_planes + "\"");
  }
  if (!dump_u.empty()) {
    std::vector<double> u(n);
    cvh_check(ctx, cvh_get_levelset(ctx, u.data()), "cvh_get_levelset");
    std::ofstream out(dump_u, std::ios::binary);
    out.write(reinterpret_cast<const char *>(u.data()), (std::streamsize)(n * sizeof(double)));
    if (!out) msg_exit("Error: cannot write \"" + dump_u + "\"");
  }
  // --morph: the cleaned mask (-I applied as invert), morphed, becomes the level set on the device -- behind --dump-u, --energy and
  // --truth, which speak of the run's own level set; everything below then reads the result as a plain mask
  if (morph_op != CVH_MORPH_NONE) {
    cvh_check(ctx, cvh_morph_levelset(ctx, connectivity, invert ? 1 : 0, min_area, fill_holes, largest ? 1 : 0, morph_op, morph_r2, 1.0, -1.0),
              "cvh_morph_levelset");
    invert = false; min_area = 0; fill_holes = 0; largest = false; clean_mask = false;
  }
  // --truth-labels: the components of the mask --dump-mask uses against the objects of the label image, read off one table
  if (!truth_labels.empty()) {
    long pairs = 0;
    const int inv = invert ? 1 : 0, big = largest ? 1 : 0;
    cvh_check(ctx, cvh_overlaps(ctx, connectivity, inv, min_area, fill_holes, big, truth_labels.data(), nullptr, 0, &pairs, nullptr), "cvh_overlaps");
    std::vector<cvh_overlap> table((size_t)pairs);
    cvh_check(ctx, cvh_overlaps(ctx, connectivity, inv, min_area, fill_holes, big, truth_labels.data(), table.data(), pairs, &pairs, nullptr),
              "cvh_overlaps");
    cvh_match half;
    if (cvh_match_overlaps(table.data(), pairs, 1, 2, nullptr, 0, &half) != CVH_OK) msg_exit("Error: cvh_match_overlaps refused the table");
    double mean_ap = 0.0;
    const double objects = (double)half.objects_a + (double)half.objects_b;
    for (uint32_t t = 10; t < 20; ++t) {
      cvh_match m;
      if (cvh_match_overlaps(table.data(), pairs, t, 20, nullptr, 0, &m) != CVH_OK) msg_exit("Error: cvh_match_overlaps refused the table");
      mean_ap += (double)m.tp / (objects - (double)m.tp);   // (tp + fp + fn = objects_a + objects_b - tp)
    }
    mean_ap = objects != 0.0 ? mean_ap / 10.0 : std::numeric_limits<double>::quiet_NaN();
    std::printf("objects: objects_a=%u objects_b=%u tp=%u fp=%u fn=%u mean_ap=%.17g\n", half.objects_a, half.objects_b, half.tp, half.fp, half.fn,
                mean_ap);
  }
  // the cleaned mask (-I applied as invert), where a cleaning option was given: what --dump-mask, _selection and --roi then use
  std::vector<uint8_t> cleaned;
  if (clean_mask && (!dump_mask.empty() || object_selection || roi)) {
    cleaned.resize(n);
    cvh_check(ctx, cvh_get_mask_clean(ctx, cleaned.data(), connectivity, invert ? 1 : 0, min_area, fill_holes, largest ? 1 : 0), "cvh_get_mask_clean");
  }
  if (!dump_mask.empty()) {
    std::vector<uint8_t> m(n);
    if (clean_mask) m = cleaned;
    else cvh_check(ctx, cvh_get_mask(ctx, m.data(), invert ? 1 : 0), "cvh_get_mask");
    for (auto &v : m) v = v ? 255 : 0;
    if (!write_image(dump_mask, h, w, 1, m.data())) msg_exit("Error: cannot write \"" + dump_mask + "\"");
  }

  if (!measure_filename.empty()) {   // the components of that mask, measured on the device: one CSV line each
    int count = 0;
    cvh_check(ctx, cvh_measure(ctx, connectivity, invert ? 1 : 0, min_area, fill_holes, largest ? 1 : 0, nullptr, 0, &count, nullptr), "cvh_measure");
    std::vector<cvh_region> table((size_t)count);
    if (count)
      cvh_check(ctx, cvh_measure(ctx, connectivity, invert ? 1 : 0, min_area, fill_holes, largest ? 1 : 0, table.data(), count, &count, nullptr), "cvh_measure");
    FILE *f = std::fopen(measure_filename.c_str(), "w");
    if (!f) msg_exit("Error: cannot write \"" + measure_filename + "\"");
    std::fprintf(f, "label,first,area,x0,y0,x1,y1,border,perimeter,cx,cy,mu20,mu02,mu11,theta,major,minor");
    for (const char *name : {"mean", "var"})
      for (int k = 0; k < run_channels; ++k) std::fprintf(f, ",%s%d", name, k);
    std::fprintf(f, "\n");
    for (int k = 0; k < count; ++k) {
      const cvh_region &r = table[(size_t)k];
      cvh_region_shape s;
      if (cvh_region_shape_of(&r, run_channels, &s) != CVH_OK) msg_exit("Error: cvh_region_shape_of refused row " + std::to_string(k));
      std::fprintf(f, "%d,%u,%u,%d,%d,%d,%d,%u,%llu,%.17g,%.17g,%.17g,%.17g,%.17g,%.17g,%.17g,%.17g", k + 1, r.first, r.area, r.x0, r.y0, r.x1, r.y1,
                   r.border, (unsigned long long)r.perimeter, s.cx, s.cy, s.mu20, s.mu02, s.mu11, s.theta, s.major, s.minor);
      for (int j = 0; j < run_channels; ++j) std::fprintf(f, ",%.17g", s.mean[j]);
      for (int j = 0; j < run_channels; ++j) std::fprintf(f, ",%.17g", s.var[j]);
      std::fprintf(f, "\n");
    }
    if (std::fclose(f) != 0) msg_exit("Error: cannot write \"" + measure_filename + "\"");
  }

  if (!contours_filename.empty() && contours_subpixel) {   // the zero level as ordered closed polygons: the same lines, a point per edge
    long nloops = 0, npoints = 0;
    cvh_check(ctx, cvh_contours_subpixel(ctx, connectivity, invert ? 1 : 0, min_area, fill_holes, largest ? 1 : 0, nullptr, 0, nullptr, 0, &nloops, &npoints),
              "cvh_contours_subpixel");
    std::vector<cvh_contour_loop> loops((size_t)nloops);
    std::vector<double> points(2 * (size_t)npoints);
    if (nloops)
      cvh_check(ctx, cvh_contours_subpixel(ctx, connectivity, invert ? 1 : 0, min_area, fill_holes, largest ? 1 : 0, loops.data(), nloops, points.data(),
                                           npoints, &nloops, &npoints), "cvh_contours_subpixel");
    FILE *f = std::fopen(contours_filename.c_str(), "w");
    if (!f) msg_exit("Error: cannot write \"" + contours_filename + "\"");
    for (const cvh_contour_loop &l : loops) {
      std::fprintf(f, "%u %u %lld :", l.first, l.edges, (long long)l.area2);
      for (uint64_t q = l.offset; q < l.offset + l.points; ++q) std::fprintf(f, " %.17g,%.17g", points[2 * q], points[2 * q + 1]);
      std::fprintf(f, "\n");
    }
    if (std::fclose(f) != 0) msg_exit("Error: cannot write \"" + contours_filename + "\"");
  } else if (!contours_filename.empty()) {   // the boundary of that mask as ordered closed loops, traced on the device: one text line each
    const int simplify = contours_all ? 0 : 1;
    long nloops = 0, npoints = 0;
    cvh_check(ctx, cvh_contours(ctx, connectivity, invert ? 1 : 0, min_area, fill_holes, largest ? 1 : 0, simplify, nullptr, 0, nullptr, 0, &nloops, &npoints),
              "cvh_contours");
    std::vector<cvh_contour_loop> loops((size_t)nloops);
    std::vector<int32_t> points(2 * (size_t)npoints);
    if (nloops)
      cvh_check(ctx, cvh_contours(ctx, connectivity, invert ? 1 : 0, min_area, fill_holes, largest ? 1 : 0, simplify, loops.data(), nloops, points.data(),
                                  npoints, &nloops, &npoints), "cvh_contours");
    FILE *f = std::fopen(contours_filename.c_str(), "w");
    if (!f) msg_exit("Error: cannot write \"" + contours_filename + "\"");
    for (const cvh_contour_loop &l : loops) {
      std::fprintf(f, "%u %u %lld :", l.first, l.edges, (long long)l.area2);
      for (uint64_t q = l.offset; q < l.offset + l.points; ++q) std::fprintf(f, " %d,%d", points[2 * q], points[2 * q + 1]);
      std::fprintf(f, "\n");
    }
    if (std::fclose(f) != 0) msg_exit("Error: cannot write \"" + contours_filename + "\"");
  }

  // ---- selection: src/main.cpp:1004-1005
  if (object_selection) {
    std::vector<uint8_t> sel(n * 3), rgb(n * 3);
    if (clean_mask) {   // separate()'s rule (src/main.cpp:386-405) on the cleaned mask: white canvas, the image copied where the mask is set
      for (size_t q = 0; q < n; ++q)
        for (int k = 0; k < 3; ++k) sel[3 * q + k] = cleaned[q] ? img_bgr[3 * q + k] : 255;
    } else {
      cvh_check(ctx, cvh_separate(ctx, img_bgr.data(), invert ? 1 : 0, sel.data()), "cvh_separate");
    }
    for (size_t q = 0; q < n; ++q) { rgb[3 * q] = sel[3 * q + 2]; rgb[3 * q + 1] = sel[3 * q + 1]; rgb[3 * q + 2] = sel[3 * q]; }
    if (!write_image(add_suffix(input_filename, "selection"), h, w, 3, rgb.data()))
      msg_exit("Error: cannot write \"" + add_suffix(input_filename, "selection") + "\"");
  }
  if (roi) {   // the largest component of the mask the other outputs use (ties: the smaller first index), "roi none" for an empty mask
    std::vector<uint8_t> m(n);
    if (largest) m = cleaned;
    else cvh_check(ctx, cvh_get_mask_clean(ctx, m.data(), connectivity, invert ? 1 : 0, min_area, fill_holes, 1), "cvh_get_mask_clean");
    long x0 = w, y0 = h, x1 = -1, y1 = -1, area = 0;
    for (int i = 0; i < h; ++i)
      for (int j = 0; j < w; ++j)
        if (m[(size_t)i * w + j]) { x0 = std::min<long>(x0, j); x1 = std::max<long>(x1, j); y0 = std::min<long>(y0, i); y1 = std::max<long>(y1, i); ++area; }
    if (area) std::printf("roi %ld %ld %ld %ld %ld\n", x0, y0, x1, y1, area);
    else std::printf("roi none\n");
  }
  if (vm.count("verbose"))  // the reference prints nothing
    std::fprintf(stderr, "chan_vese: %d iterations, last ||u_diff|| = %.17g\n", steps_done, last_norm);
  if (vm.count("verbose") && levels > 1) {
    std::fprintf(stderr, "chan_vese: iterations per level, finest first:");
    for (int s : level_steps) std::fprintf(stderr, " %d", s);
    std::fprintf(stderr, "\n");
  }
  if (local && rank) cvh_destroy(ranked);
  if (local || rank) cvh_destroy(ingest);
  for (int k = levels - 1; k >= 0; --k) cvh_destroy(level[k]);
  return EXIT_SUCCESS;
}
