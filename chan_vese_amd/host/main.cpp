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
// --levels, --energy, --energy-every, --truth, --score-tol, --measure, --contours, --contours-all, --contours-subpixel, --morph, --morph-radius, --init-mask, --truth-labels, --phases, --init2, --dump-labels, --localized, --split, --split-labels (--split R: cvh_split_levelset, "Object split", bakes a cut between touching objects in front of the mask outputs; --split-labels FILE: the labels as raw int32; both are listed by --help --verbose, the plain --help being pinned; --localized R: cvh_localized_run, "Localised regions"; --phases 4: chanvese_hip.h, "Four phases" -- two contexts, cvh_multiphase_run, the labels; what does not compose with it is refused).  --truth-labels FILE
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
// --smooth blur|detail with --smooth-sigma S (chanvese_hip.h, "Smoothing"): the run iterates on the Gaussian blur of every plane, or on
// 128 + plane - blur; made on the device behind --rank and in front of --local.  --edge-sigma S (with --edge K): the edge map is built
// from a blurred scratch copy of the planes; the taps of both are cvh_gauss_taps'.
// --colorspace ycrcb|yuv (chanvese_hip.h, "Colour spaces"; not with -g): the loader's B, G, R planes become (Y, Cr, Cb) / (Y, U, V) on the
// device behind Perona-Malik -- <stem>_pm stays the RGB picture the reference writes -- and in front of the iterations (with --levels: on
// the finest level, before the restricts); --lambda1 / --lambda2 then weigh the luma and the two chroma planes, a start of --init otsu /
// --threshold is taken again from the converted planes, and nothing is converted back: frames, _selection and _contour use the input.
// The stages, in main()'s order: read_options (options.hpp), load_inputs, the parameters, then either run_four_phase or make_run,
// the first start, the t = 0 frame, smooth_and_write_pm, convert_colour, iterate, the reports, split_objects (--split) or the morph
// bake, and the mask outputs.
// --convex TAU[,SIGMA] with --convex-means M and --convex-stop S runs the convex relaxation of the two-phase model by primal-dual
// iterations from the mask of the start (chanvese_hip.h, "Convex relaxation": cvh_convex_run in place of cvh_run), with --edge K the
// weighted model on the edge map; the level set written is v - 1/2.
#include <algorithm>
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <limits>
#include <string>
#include <vector>

#include <sys/stat.h>

#include "chanvese_hip.h"
#include "image_io.hpp"
#include "options.hpp"
#include "overlay_text.hpp"

namespace {

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

void cvh_check(cvh_context *ctx, int rc, const char *what)
{
  if (rc != CVH_OK) msg_exit(std::string("Error: ") + what + ": " + cvh_last_error(ctx));
}

// ---- writers that end the program where the file cannot be written
[[noreturn]] void cannot_write(const std::string &path) { msg_exit("Error: cannot write \"" + path + "\""); }

void write_or_exit(const std::string &path, int h, int w, int channels, const uint8_t *px)
{
  if (!write_image(path, h, w, channels, px)) cannot_write(path);
}

void write_raw_or_exit(const std::string &path, const void *data, size_t bytes)
{
  std::ofstream out(path, std::ios::binary);
  out.write(reinterpret_cast<const char *>(data), (std::streamsize)bytes);
  if (!out) cannot_write(path);
}

struct TextFile {   // a text output: opened, printed to through f, closed
  std::string path;
  FILE *f;
  explicit TextFile(const std::string &p) : path(p), f(std::fopen(p.c_str(), "w")) { if (!f) cannot_write(path); }
  void close() { if (std::fclose(f) != 0) cannot_write(path); }
};

// ---- the mask-source calls of the library take the five cleaning values in one order
template <class F, class... Rest> int with_clean(F call, cvh_context *ctx, const CleanArgs &c, Rest... rest)
{
  return call(ctx, c.conn, c.invert, c.min_area, c.fill_holes, c.largest, rest...);
}

void get_mask_clean(cvh_context *ctx, const CleanArgs &c, uint8_t *mask)
{
  cvh_check(ctx, cvh_get_mask_clean(ctx, mask, c.conn, c.invert, c.min_area, c.fill_holes, c.largest), "cvh_get_mask_clean");
}

// ---- inputs: src/main.cpp:877-887 (8-bit gray or BGR) and the side files of this build
struct Inputs {
  int h = 0, w = 0;
  size_t n = 0;
  bool input_is_png = false;
  std::vector<uint8_t> img_bgr;                // what the reference calls `img` (3 channels, BGR)
  std::vector<std::vector<uint8_t>> planes;    // what cv::split leaves (:934-937); Perona-Malik's result is read back into them
  std::vector<uint8_t> truth;                  // --truth: one byte per pixel, non-zero = foreground
  std::vector<int32_t> truth_labels;           // --truth-labels: one label per pixel
  std::vector<uint8_t> init_mask;              // --init-mask: one byte per pixel, non-zero = inside
  std::vector<uint8_t *> plane_pointers()
  {
    std::vector<uint8_t *> pp;
    for (auto &p : planes) pp.push_back(p.data());
    return pp;
  }
};

void same_size_or_exit(const char *noun, const std::string &path, int h, int w, const Inputs &in)
{
  if (h != in.h || w != in.w)
    msg_exit(std::string("The ") + noun + " \"" + path + "\" is " + std::to_string(w) + " x " + std::to_string(h) + ", the input " +
             std::to_string(in.w) + " x " + std::to_string(in.h) + ": they must have the same size.");
}

Inputs load_inputs(const Options &opt)
{
  Inputs in;
  Image file;
  if (!read_image(opt.input, file, in.input_is_png)) msg_exit("Error on opening \"" + opt.input + "\" (probably not an image)!");
  if (!in.input_is_png && has_ext(opt.input, ".png")) msg_exit("Error on opening \"" + opt.input + "\" (probably not an image)!");
  in.h = file.h; in.w = file.w;
  const size_t n = in.n = (size_t)file.h * file.w;
  if (!opt.truth.empty()) {
    Image t;
    bool truth_is_png = false;
    if (!read_image(opt.truth, t, truth_is_png)) msg_exit("Error on opening \"" + opt.truth + "\" (probably not an image)!");
    same_size_or_exit("ground truth", opt.truth, t.h, t.w, in);
    in.truth.resize(n);
    for (size_t q = 0; q < n; ++q) {
      uint8_t any = 0;
      for (int k = 0; k < t.channels; ++k) any |= t.px[(size_t)t.channels * q + k];
      in.truth[q] = any;
    }
  }
  if (!opt.truth_labels.empty()) {
    int th = 0, tw = 0;
    if (!read_labels(opt.truth_labels, th, tw, in.truth_labels))
      msg_exit("Error on opening \"" + opt.truth_labels + "\" (a label image must be a binary PGM with maxval <= 65535 or an 8-bit grey PNG)!");
    same_size_or_exit("label image", opt.truth_labels, th, tw, in);
  }
  if (!opt.init_mask.empty()) {
    Image t;
    if (!read_pnm(opt.init_mask, t) || t.channels != 1) msg_exit("Error on opening \"" + opt.init_mask + "\" (a mask start must be a binary PGM)!");
    same_size_or_exit("mask start", opt.init_mask, t.h, t.w, in);
    in.init_mask.assign(t.px.begin(), t.px.begin() + (std::ptrdiff_t)n);
  }
  in.img_bgr.resize(n * 3);
  in.planes.assign((size_t)opt.nof_channels(), std::vector<uint8_t>(n));
  for (size_t q = 0; q < n; ++q) {
    uint8_t b, g, r;
    if (file.channels == 1) { b = g = r = file.px[q]; }
    else { r = file.px[3 * q]; g = file.px[3 * q + 1]; b = file.px[3 * q + 2]; }
    if (opt.grayscale) {
      // cv::imread(..., GRAYSCALE) of a colour file.  PxM decoder: icvCvt_BGR2Gray_8u_C3C1R, 14-bit fixed
      // point BT.601 (R 4899, G 9617, B 1868).  PNG decoder: libpng's png_set_rgb_to_gray(0.299, 0.587),
      // 15-bit fixed point (R 9798, G 19235, B 3735, rounded; equal channels pass through).
      uint8_t y;
      if (file.channels == 1) y = b;
      else if (!in.input_is_png) y = (uint8_t)((r * 4899 + g * 9617 + b * 1868 + 8192) >> 14);
      else y = (r == g && g == b) ? r : (uint8_t)((r * 9798 + g * 19235 + b * 3735 + 16384) >> 15);
      in.img_bgr[3 * q] = in.img_bgr[3 * q + 1] = in.img_bgr[3 * q + 2] = y;  // cvtColor GRAY2RGB (:885)
      in.planes[0][q] = y;
    } else {
      in.img_bgr[3 * q] = b; in.img_bgr[3 * q + 1] = g; in.img_bgr[3 * q + 2] = r;
      in.planes[0][q] = b; in.planes[1][q] = g; in.planes[2][q] = r;
    }
  }
  return in;
}

// ---- contexts
struct ContextOptions {
  int math_mode = -1;        // -1: the library's default
  int state = 64;
  bool state_may_fail = false;   // a helper level too narrow for FP32 state keeps 64
  int co_resident = -1;      // -1: the library's default
};

cvh_context *make_context(int h, int w, int channels, const cvh_params *prm, int device, const ContextOptions &co)
{
  cvh_context *c = nullptr;
  if (cvh_create(&c, h, w, channels, prm, device) != CVH_OK)
    msg_exit(std::string("Error: cannot initialise the HIP backend: ") + cvh_last_error(nullptr));
  if (co.math_mode >= 0) cvh_check(c, cvh_set_option(c, "math_mode", co.math_mode), "math_mode");
  if (co.state == 32) {   // declared FP32-state mode: never the default
    const int rc = cvh_set_option(c, "state", 32);
    if (!co.state_may_fail) cvh_check(c, rc, "state");
  }
  if (co.co_resident >= 0) cvh_check(c, cvh_set_option(c, "co_resident", co.co_resident), "co_resident");
  return c;
}

// The contexts of a run.  level[0] = ctx is the one that runs and that every output reads; level[1..] are the helper levels of a
// coarse-to-fine run, each half the one before (idle while another level runs: "co_resident"), or the second level set of a four-phase
// run.  --local: the file's planes go into a context of their own (ingest), where they are smoothed and converted; ctx receives their
// local statistics.  --rank goes the same way and in front of --local: with both, the rank planes land in a context of their own
// (ranked) that --local reads.  --smooth stands between the two: the stages run rank, smooth, local, each reading what the one before
// made; the last one writes ctx, the others a context of their own (ranked, smoothed).
struct Run {
  const Options &opt;
  cvh_context *ctx = nullptr, *ingest = nullptr, *ranked = nullptr, *smoothed = nullptr;
  std::vector<cvh_context *> level;
  explicit Run(const Options &o) : opt(o) {}
  Run(const Run &) = delete;
  void refresh_planes() const   // ctx's planes from ingest's: at the start, and again behind -S and --colorspace
  {
    cvh_context *made = ingest;   // where the last stage has left the planes
    if (opt.rank) { cvh_check(ranked, cvh_rank_planes(made, ranked, opt.rank_radius, opt.rank_what), "cvh_rank_planes"); made = ranked; }
    if (opt.smooth) {
      cvh_check(smoothed, cvh_smooth_planes(made, smoothed, opt.smooth_radius, opt.smooth_taps, opt.smooth_what), "cvh_smooth_planes");
      made = smoothed;
    }
    if (opt.local) cvh_check(ctx, cvh_local_planes(made, ctx, opt.local_radius, opt.local_what), "cvh_local_planes");
  }
  ~Run()
  {
    if (smoothed != ctx) cvh_destroy(smoothed);
    if (ranked != ctx) cvh_destroy(ranked);
    if (ingest != ctx) cvh_destroy(ingest);
    for (size_t k = level.size(); k-- > 0;) cvh_destroy(level[k]);
  }
};

void make_run(Run &run, const Options &opt, Inputs &in, const cvh_params &prm)
{
  std::vector<std::pair<int, int>> shape{{in.h, in.w}};   // finest first
  for (int k = 1; k < opt.levels; ++k) shape.push_back({(shape.back().first + 1) / 2, (shape.back().second + 1) / 2});
  if (std::min(shape.back().first, shape.back().second) < 16 && opt.levels > 1)
    msg_exit("Too many levels for a " + std::to_string(in.h) + " x " + std::to_string(in.w) + " image: the coarsest side must not fall below 16.");
  ContextOptions co;
  co.math_mode = opt.math_mode; co.state = opt.state_bits;
  run.ctx = run.ingest = run.ranked = run.smoothed = make_context(in.h, in.w, opt.run_channels(), &prm, opt.device, co);
  run.level.push_back(run.ctx);
  co.state_may_fail = true; co.co_resident = 0;
  for (int k = 1; k < opt.levels; ++k) run.level.push_back(make_context(shape[k].first, shape[k].second, opt.run_channels(), &prm, opt.device, co));
  ContextOptions planes_only;
  planes_only.co_resident = 0;
  if (opt.local || opt.rank || opt.smooth) run.ingest = make_context(in.h, in.w, opt.nof_channels(), nullptr, opt.device, planes_only);
  if (opt.rank && (opt.smooth || opt.local)) run.ranked = make_context(in.h, in.w, opt.nof_channels(), nullptr, opt.device, planes_only);
  if (opt.smooth && opt.local) run.smoothed = make_context(in.h, in.w, opt.nof_channels(), nullptr, opt.device, planes_only);
  cvh_check(run.ingest, cvh_set_image(run.ingest, in.plane_pointers().data()), "cvh_set_image");
  run.refresh_planes();
}

// ---- level set: src/main.cpp:898-923.  The starts built on the device take their numbers shifted right by `shift` (a coarse-to-fine
// run builds its start on the coarsest level)
void start_levelset(cvh_context *c, const Start &s, const Options &opt, const Inputs &in, int shift = 0)
{
  switch (s.kind) {
  case Start::Rect:   // src/InteractiveDataRect.cpp:24-25
    cvh_check(c, cvh_init_rect(c, opt.rx >> shift, opt.ry >> shift, opt.rw >> shift, opt.rh >> shift, 1.0, 0.0), "cvh_init_rect");
    break;
  case Start::Disk:
    cvh_check(c, cvh_init_disk(c, opt.disk_cx >> shift, opt.disk_cy >> shift, opt.disk_r >> shift, 1.0, 0.0), "cvh_init_disk");
    break;
  case Start::Otsu: cvh_check(c, cvh_init_otsu(c, nullptr, 1.0, -1.0), "cvh_init_otsu"); break;
  case Start::Threshold: cvh_check(c, cvh_init_threshold(c, s.threshold, 1.0, -1.0), "cvh_init_threshold"); break;
  case Start::Mask: cvh_check(c, cvh_init_mask(c, in.init_mask.data(), 1.0, -1.0), "cvh_init_mask"); break;
  case Start::Circ: {
    if (!opt.circ_ok) msg_exit("You must specify the contour with non-zero dimensions");
    std::vector<double> u(in.n, 0.0);  // src/InteractiveDataCirc.cpp:23-24
    draw_circle_outline(u, in.h, in.w, opt.cx, opt.cy, opt.cr);
    cvh_check(c, cvh_set_levelset(c, u.data()), "cvh_set_levelset");
    break;
  }
  case Start::Checkerboard: cvh_check(c, cvh_init_checkerboard(c), "cvh_init_checkerboard"); break;
  case Start::Rolled: {   // the checkerboard rolled by (2, 3) pixels: two identical starts would stay identical forever
    std::vector<double> cb(in.n), u2(in.n);
    cvh_levelset_checkerboard_host(in.h, in.w, cb.data());
    for (int i = 0; i < in.h; ++i)
      for (int j = 0; j < in.w; ++j) u2[(size_t)((i + 2) % in.h) * in.w + (size_t)((j + 3) % in.w)] = cb[(size_t)i * in.w + j];
    cvh_check(c, cvh_set_levelset(c, u2.data()), "cvh_set_levelset");
    break;
  }
  }
}

// a start taken from the image is taken again from the changed planes: behind -S and behind --colorspace
void restart_from_image(const Run &run, const Options &opt, const Inputs &in)
{
  if (opt.levels == 1 && opt.start.from_image()) start_levelset(run.ctx, opt.start, opt, in);
}

// ---- Perona-Malik: src/main.cpp:940-947; the smoothed bytes come back into in.planes and go out as <stem>_pm
void smooth_and_write_pm(const Run &run, const Options &opt, Inputs &in)
{
  cvh_check(run.ingest, cvh_perona_malik(run.ingest, opt.K, opt.L, opt.T), "cvh_perona_malik");
  cvh_check(run.ingest, cvh_get_image(run.ingest, in.plane_pointers().data()), "cvh_get_image");
  run.refresh_planes();
  const int channels = opt.nof_channels();
  std::vector<uint8_t> out(in.n * channels);
  for (size_t q = 0; q < in.n; ++q) {
    if (channels == 1) out[q] = in.planes[0][q];
    else { out[3 * q] = in.planes[2][q]; out[3 * q + 1] = in.planes[1][q]; out[3 * q + 2] = in.planes[0][q]; }  // BGR -> RGB file order
  }
  write_or_exit(add_suffix(opt.input, "pm"), in.h, in.w, channels, out.data());
}

// ---- video frames: src/main.cpp:926-931; VideoWriterManager::write_frame, src/VideoWriterManager.cpp:40-57
struct Frames {
  std::string dir, ext;
  int frame_no = 0;
  std::vector<uint8_t> contour, frame;
  explicit Frames(const std::string &input)
  {
    const size_t dot = input.find_last_of('.');
    const size_t slash = input.find_last_of('/');
    const bool with_ext = dot != std::string::npos && (slash == std::string::npos || dot > slash + 1);
    dir = (with_ext ? input.substr(0, dot) : input) + "_frames";
    ext = with_ext && has_ext(input.substr(dot), ".png") ? ".png" : ".ppm";
  }
  void write(cvh_context *ctx, const Options &opt, const Inputs &in, const std::string &txt)
  {
    contour.resize(in.n); frame.resize(in.n * 3);
    cvh_check(ctx, cvh_get_contour(ctx, contour.data()), "cvh_get_contour");
    for (size_t q = 0; q < in.n; ++q) {   // frames are RGB files; img_bgr is the reference's `img`
      const bool c = contour[q] != 0;
      frame[3 * q] = c ? opt.contour_bgr[2] : in.img_bgr[3 * q + 2];
      frame[3 * q + 1] = c ? opt.contour_bgr[1] : in.img_bgr[3 * q + 1];
      frame[3 * q + 2] = c ? opt.contour_bgr[0] : in.img_bgr[3 * q];
    }
    if (opt.overlay_text && !txt.empty()) {   // :47-53: colour and corner from overlay_color (:76-114), own 5x7 glyphs
      int px, py; bool black;
      overlay::place(in.img_bgr.data(), in.h, in.w, txt, opt.overlay_pos, &px, &py, &black);
      overlay::draw(frame.data(), in.h, in.w, txt, px, py, black);
    }
    char name[64];
    std::snprintf(name, sizeof(name), "/frame_%06d", frame_no++);
    write_or_exit(dir + name + ext, in.h, in.w, 3, frame.data());
  }
};

// ---- timestep loop: src/main.cpp:950-1001 (stop condition and every iteration on the GPU)
struct Progress {
  int steps = 0;
  double norm = 0;
  std::vector<int> level_steps;   // iterations per level, finest first
};

void energy_line(cvh_context *ctx, int channels, int iteration)   // "[iteration ]energy total length area fit_in... fit_out...", every number %.17g
{
  cvh_energy_terms e;
  cvh_check(ctx, cvh_energy(ctx, &e), "cvh_energy");
  if (iteration >= 0) std::printf("%d ", iteration);
  std::printf("energy %.17g %.17g %.17g", e.total, e.length, e.area);
  for (int k = 0; k < channels; ++k) std::printf(" %.17g", e.fit_in[k]);
  for (int k = 0; k < channels; ++k) std::printf(" %.17g", e.fit_out[k]);
  std::printf("\n");
  std::fflush(stdout);
}

// one iteration per frame; the frame is saved before the stop test (:997-1000)
void run_with_frames(cvh_context *ctx, const Options &opt, const Inputs &in, Frames &frames, Progress &p)
{
  for (int t = 1; t <= opt.steps(); ++t) {
    int stopped = 0;
    cvh_check(ctx, cvh_enqueue_steps(ctx, 1), "cvh_enqueue_steps");
    cvh_check(ctx, cvh_sync(ctx, &p.steps, &p.norm, &stopped), "cvh_sync");
    frames.write(ctx, opt, in, "t = " + std::to_string(t));   // :997
    if (stopped) break;
  }
}

// segments of `every` iterations with after(stopped, left) behind each; a stop inside a segment ends the run
template <class After> void run_in_segments(cvh_context *ctx, int every, int max_steps, Progress &p, After after)
{
  for (int left = max_steps; left > 0;) {
    const int k = std::min(every, left);
    int done = 0, stopped = 0;
    cvh_check(ctx, cvh_run(ctx, k, &done, &p.norm), "cvh_run");
    cvh_check(ctx, cvh_sync(ctx, nullptr, nullptr, &stopped), "cvh_sync");
    p.steps += done;
    left -= k;
    after(stopped != 0, left);
    if (stopped) break;
  }
}

// restrict down the chain, start on the coarsest level, then level by level: run, prolong.  While a level runs the others do not
// count in its automatic choices ("co_resident"); the finest keeps its own value throughout
void run_coarse_to_fine(const Run &run, const Options &opt, const Inputs &in, Frames &frames, Progress &p)
{
  const std::vector<cvh_context *> &level = run.level;
  const int levels = opt.levels;
  for (int k = 0; k + 1 < levels; ++k) cvh_check(level[k + 1], cvh_restrict_image(level[k], level[k + 1]), "cvh_restrict_image");
  start_levelset(level.back(), opt.start, opt, in, levels - 1);
  for (int k = levels - 1; k >= 0; --k) {
    if (k + 1 < levels) cvh_check(level[k], cvh_prolong_levelset(level[k + 1], level[k]), "cvh_prolong_levelset");
    if (k > 0) {
      cvh_check(level[k], cvh_set_option(level[k], "co_resident", 1), "co_resident");
      cvh_check(level[k], cvh_run(level[k], opt.steps(), &p.level_steps[k], nullptr), "cvh_run");
      cvh_check(level[k], cvh_set_option(level[k], "co_resident", 0), "co_resident");
    } else if (!opt.video) {
      cvh_check(run.ctx, cvh_run(run.ctx, opt.steps(), &p.steps, &p.norm), "cvh_run");
    } else {
      frames.write(run.ctx, opt, in, "t = 0");
      run_with_frames(run.ctx, opt, in, frames, p);
    }
  }
  p.level_steps[0] = p.steps;
}

Progress iterate(const Run &run, const Options &opt, const Inputs &in, Frames &frames)
{
  cvh_context *ctx = run.ctx;
  Progress p;
  p.level_steps.assign((size_t)opt.levels, 0);
  if (opt.levels > 1) {
    run_coarse_to_fine(run, opt, in, frames, p);
  } else if (opt.reinit_every > 0) {   // the level set re-distanced between the segments
    run_in_segments(ctx, opt.reinit_every, opt.steps(), p, [&](bool stopped, int left) {
      if (!stopped && left > 0) cvh_check(ctx, cvh_reinit(ctx, nullptr), "cvh_reinit");
    });
  } else if (opt.energy_every > 0) {   // the energy taken behind each segment
    run_in_segments(ctx, opt.energy_every, opt.steps(), p, [&](bool, int) { energy_line(ctx, opt.run_channels(), p.steps); });
  } else if (opt.localized) {
    cvh_check(ctx, cvh_localized_run(ctx, opt.localized, opt.steps(), &p.steps, &p.norm, nullptr, 0, nullptr), "cvh_localized_run");
  } else if (opt.edge > 0.0) {   // the map from the planes as every stage in front of the run has left them
    if (opt.edge_sigma > 0.0) {   // g from G_sigma * I: a blurred scratch copy is the map's source, the run keeps the planes
      ContextOptions planes_only;
      planes_only.co_resident = 0;
      cvh_context *scratch = make_context(in.h, in.w, opt.run_channels(), nullptr, opt.device, planes_only);
      const int blur[3] = {CVH_SMOOTH_BLUR, CVH_SMOOTH_BLUR, CVH_SMOOTH_BLUR};
      cvh_check(scratch, cvh_smooth_planes(ctx, scratch, opt.edge_radius, opt.edge_taps, blur), "cvh_smooth_planes");
      cvh_check(ctx, cvh_edge_map(ctx, scratch, opt.edge), "cvh_edge_map");
      cvh_destroy(scratch);
    } else {
      cvh_check(ctx, cvh_edge_map(ctx, ctx, opt.edge), "cvh_edge_map");
    }
    if (!opt.dump_edge.empty()) {
      std::vector<uint16_t> gq(in.n);
      cvh_check(ctx, cvh_get_edge_map(ctx, gq.data()), "cvh_get_edge_map");
      write_raw_or_exit(opt.dump_edge, gq.data(), in.n * sizeof(uint16_t));
    }
    if (opt.convex) cvh_check(ctx, cvh_convex_run(ctx, opt.steps(), &opt.convex_params, &p.steps, &p.norm, nullptr, 0, nullptr), "cvh_convex_run");
    else cvh_check(ctx, cvh_geodesic_run(ctx, opt.steps(), &p.steps, &p.norm, nullptr, 0, nullptr), "cvh_geodesic_run");
  } else if (opt.convex) {
    cvh_check(ctx, cvh_convex_run(ctx, opt.steps(), &opt.convex_params, &p.steps, &p.norm, nullptr, 0, nullptr), "cvh_convex_run");
  } else if (!opt.video) {
    cvh_check(ctx, cvh_run(ctx, opt.steps(), &p.steps, &p.norm), "cvh_run");
  } else {
    run_with_frames(ctx, opt, in, frames, p);
  }
  return p;
}

// ---- reports and outputs, in main()'s order
// --truth: the derived figures as the header spells them; nan where a denominator is 0 or a surface is empty
void print_score(cvh_context *ctx, const Options &opt, const Inputs &in)
{
  cvh_mask_score s;
  cvh_check(ctx, cvh_score_mask(ctx, in.truth.data(), opt.clean.invert, opt.score_tol2, &s), "cvh_score_mask");
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

// --dump-planes: the planes the run iterated on, one under the other
void dump_planes(cvh_context *ctx, const Options &opt, const Inputs &in)
{
  const int channels = opt.run_channels();
  std::vector<uint8_t> all(in.n * channels);
  std::vector<uint8_t *> pp;
  for (int k = 0; k < channels; ++k) pp.push_back(all.data() + (size_t)k * in.n);
  cvh_check(ctx, cvh_get_image(ctx, pp.data()), "cvh_get_image");
  write_or_exit(opt.dump_planes, in.h * channels, in.w, 1, all.data());
}

void dump_levelset(cvh_context *ctx, const Options &opt, const Inputs &in)
{
  std::vector<double> u(in.n);
  cvh_check(ctx, cvh_get_levelset(ctx, u.data()), "cvh_get_levelset");
  write_raw_or_exit(opt.dump_u, u.data(), in.n * sizeof(double));
}

// --truth-labels: the components of the mask --dump-mask uses against the objects of the label image, read off one table
void print_objects(cvh_context *ctx, const CleanArgs &clean, const Inputs &in)
{
  long pairs = 0;
  cvh_check(ctx, with_clean(cvh_overlaps, ctx, clean, in.truth_labels.data(), nullptr, 0L, &pairs, nullptr), "cvh_overlaps");
  std::vector<cvh_overlap> table((size_t)pairs);
  cvh_check(ctx, with_clean(cvh_overlaps, ctx, clean, in.truth_labels.data(), table.data(), pairs, &pairs, nullptr), "cvh_overlaps");
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

// --dump-mask: 0 / 255; `cleaned` is the cleaned mask where a cleaning option was given, else empty
void dump_mask(cvh_context *ctx, const Options &opt, const Inputs &in, const CleanArgs &clean, const std::vector<uint8_t> &cleaned)
{
  std::vector<uint8_t> m(in.n);
  if (!cleaned.empty()) m = cleaned;
  else cvh_check(ctx, cvh_get_mask(ctx, m.data(), clean.invert), "cvh_get_mask");
  for (auto &v : m) v = v ? 255 : 0;
  write_or_exit(opt.dump_mask, in.h, in.w, 1, m.data());
}

// --measure: the components of that mask, measured on the device: one CSV line each
void write_measure(cvh_context *ctx, const Options &opt, const CleanArgs &clean)
{
  const int channels = opt.run_channels();
  int count = 0;
  cvh_check(ctx, with_clean(cvh_measure, ctx, clean, nullptr, 0, &count, nullptr), "cvh_measure");
  std::vector<cvh_region> table((size_t)count);
  if (count) cvh_check(ctx, with_clean(cvh_measure, ctx, clean, table.data(), count, &count, nullptr), "cvh_measure");
  TextFile out(opt.measure);
  std::fprintf(out.f, "label,first,area,x0,y0,x1,y1,border,perimeter,cx,cy,mu20,mu02,mu11,theta,major,minor");
  for (const char *name : {"mean", "var"})
    for (int k = 0; k < channels; ++k) std::fprintf(out.f, ",%s%d", name, k);
  std::fprintf(out.f, "\n");
  for (int k = 0; k < count; ++k) {
    const cvh_region &r = table[(size_t)k];
    cvh_region_shape s;
    if (cvh_region_shape_of(&r, channels, &s) != CVH_OK) msg_exit("Error: cvh_region_shape_of refused row " + std::to_string(k));
    std::fprintf(out.f, "%d,%u,%u,%d,%d,%d,%d,%u,%llu,%.17g,%.17g,%.17g,%.17g,%.17g,%.17g,%.17g,%.17g", k + 1, r.first, r.area, r.x0, r.y0, r.x1, r.y1,
                 r.border, (unsigned long long)r.perimeter, s.cx, s.cy, s.mu20, s.mu02, s.mu11, s.theta, s.major, s.minor);
    for (int j = 0; j < channels; ++j) std::fprintf(out.f, ",%.17g", s.mean[j]);
    for (int j = 0; j < channels; ++j) std::fprintf(out.f, ",%.17g", s.var[j]);
    std::fprintf(out.f, "\n");
  }
  out.close();
}

// --contours: ordered closed loops, one text line each: "first edges area2 :" and the x,y pairs.  `call` is cvh_contours (the boundary
// of that mask, traced on the device) or cvh_contours_subpixel (the zero level, a point per edge) behind its leading arguments; it is
// asked for the counts, then for the tables
template <class Point, class Call> void write_loops(cvh_context *ctx, const std::string &path, const char *what, const char *point_format, Call call)
{
  long nloops = 0, npoints = 0;
  cvh_check(ctx, call(nullptr, 0L, nullptr, 0L, &nloops, &npoints), what);
  std::vector<cvh_contour_loop> loops((size_t)nloops);
  std::vector<Point> points(2 * (size_t)npoints);
  if (nloops) cvh_check(ctx, call(loops.data(), nloops, points.data(), npoints, &nloops, &npoints), what);
  TextFile out(path);
  for (const cvh_contour_loop &l : loops) {
    std::fprintf(out.f, "%u %u %lld :", l.first, l.edges, (long long)l.area2);
    for (uint64_t q = l.offset; q < l.offset + l.points; ++q) std::fprintf(out.f, point_format, points[2 * q], points[2 * q + 1]);
    std::fprintf(out.f, "\n");
  }
  out.close();
}

void write_contours(cvh_context *ctx, const Options &opt, const CleanArgs &clean)
{
  if (opt.contours_subpixel)
    write_loops<double>(ctx, opt.contours, "cvh_contours_subpixel", " %.17g,%.17g",
                           [&](cvh_contour_loop *loops, long loop_cap, double *points, long point_cap, long *nloops, long *npoints) {
                             return with_clean(cvh_contours_subpixel, ctx, clean, loops, loop_cap, points, point_cap, nloops, npoints);
                           });
  else
    write_loops<int32_t>(ctx, opt.contours, "cvh_contours", " %d,%d",
                            [&](cvh_contour_loop *loops, long loop_cap, int32_t *points, long point_cap, long *nloops, long *npoints) {
                              return with_clean(cvh_contours, ctx, clean, opt.contours_all ? 0 : 1, loops, loop_cap, points, point_cap, nloops, npoints);
                            });
}

// ---- selection: src/main.cpp:1004-1005
void write_selection(cvh_context *ctx, const Options &opt, const Inputs &in, const CleanArgs &clean, const std::vector<uint8_t> &cleaned)
{
  const size_t n = in.n;
  std::vector<uint8_t> sel(n * 3), rgb(n * 3);
  if (!cleaned.empty()) {   // separate()'s rule (src/main.cpp:386-405) on the cleaned mask: white canvas, the image copied where the mask is set
    for (size_t q = 0; q < n; ++q)
      for (int k = 0; k < 3; ++k) sel[3 * q + k] = cleaned[q] ? in.img_bgr[3 * q + k] : 255;
  } else {
    cvh_check(ctx, cvh_separate(ctx, in.img_bgr.data(), clean.invert, sel.data()), "cvh_separate");
  }
  for (size_t q = 0; q < n; ++q) { rgb[3 * q] = sel[3 * q + 2]; rgb[3 * q + 1] = sel[3 * q + 1]; rgb[3 * q + 2] = sel[3 * q]; }
  write_or_exit(add_suffix(opt.input, "selection"), in.h, in.w, 3, rgb.data());
}

// --roi: the largest component of the mask the other outputs use (ties: the smaller first index), "roi none" for an empty mask
void print_roi(cvh_context *ctx, const Inputs &in, CleanArgs clean, const std::vector<uint8_t> &cleaned)
{
  std::vector<uint8_t> m(in.n);
  if (clean.largest) m = cleaned;
  else { clean.largest = 1; get_mask_clean(ctx, clean, m.data()); }
  const int h = in.h, w = in.w;
  long x0 = w, y0 = h, x1 = -1, y1 = -1, area = 0;
  for (int i = 0; i < h; ++i)
    for (int j = 0; j < w; ++j)
      if (m[(size_t)i * w + j]) { x0 = std::min<long>(x0, j); x1 = std::max<long>(x1, j); y0 = std::min<long>(y0, i); y1 = std::max<long>(y1, i); ++area; }
  if (area) std::printf("roi %ld %ld %ld %ld %ld\n", x0, y0, x1, y1, area);
  else std::printf("roi none\n");
}

// --split R: the cleaned mask (-I applied as invert) taken apart on the device (chanvese_hip.h, "Object split").  --split-labels gets the
// label plane, cut pixels included; then the cut is baked into the level set -- behind --dump-u, --energy and --truth, as --morph --, and
// everything that speaks of the mask reads the split objects as a plain mask
void split_objects(cvh_context *ctx, const Options &opt, const Inputs &in)
{
  if (!opt.split_labels.empty()) {
    std::vector<int32_t> labels(in.n);
    cvh_check(ctx, with_clean(cvh_split_host, ctx, opt.clean, opt.split_r2, labels.data(), nullptr, 0, nullptr), "cvh_split_host");
    write_raw_or_exit(opt.split_labels, labels.data(), in.n * sizeof(int32_t));
  }
  cvh_check(ctx, with_clean(cvh_split_levelset, ctx, opt.clean, opt.split_r2, 1.0, -1.0), "cvh_split_levelset");
}

// Everything that speaks of the mask, for the cleaning values it is to use
void mask_outputs(cvh_context *ctx, const Options &opt, const Inputs &in, const CleanArgs &clean, bool clean_mask)
{
  if (!in.truth_labels.empty()) print_objects(ctx, clean, in);
  // the cleaned mask (-I applied as invert), where a cleaning option was given: what --dump-mask, _selection and --roi then use
  std::vector<uint8_t> cleaned;
  if (clean_mask && (!opt.dump_mask.empty() || opt.select || opt.roi)) {
    cleaned.resize(in.n);
    get_mask_clean(ctx, clean, cleaned.data());
  }
  if (!opt.dump_mask.empty()) dump_mask(ctx, opt, in, clean, cleaned);
  if (!opt.measure.empty()) write_measure(ctx, opt, clean);
  if (!opt.contours.empty()) write_contours(ctx, opt, clean);
  if (opt.select) write_selection(ctx, opt, in, clean, cleaned);
  if (opt.roi) print_roi(ctx, in, clean, cleaned);
}

// ---- four phases: two contexts hold phi1 and phi2 and the same planes; everything of this run is here
void run_four_phase(const Options &opt, Inputs &in, const cvh_params &prm)
{
  Run run(opt);
  ContextOptions co;
  co.math_mode = opt.math_mode;
  for (int k = 0; k < 2; ++k) run.level.push_back(make_context(in.h, in.w, opt.run_channels(), &prm, opt.device, co));
  cvh_context *pa = run.ctx = run.ingest = run.ranked = run.smoothed = run.level[0], *pb = run.level[1];
  cvh_check(pa, cvh_set_image(pa, in.plane_pointers().data()), "cvh_set_image");
  if (opt.segment) smooth_and_write_pm(run, opt, in);   // once: B takes the smoothed bytes
  cvh_check(pb, cvh_set_image(pb, in.plane_pointers().data()), "cvh_set_image");
  start_levelset(pa, opt.start, opt, in);
  start_levelset(pb, opt.start2, opt, in);
  int steps = 0;
  double norms[2] = {0, 0};
  if (cvh_multiphase_run(pa, pb, opt.steps(), &steps, norms, nullptr, 0, nullptr) != CVH_OK)
    msg_exit(std::string("Error: cvh_multiphase_run: ") + cvh_last_error(nullptr));
  std::vector<uint8_t> labels(in.n);
  if (cvh_multiphase_labels(pa, pb, labels.data()) != CVH_OK)
    msg_exit(std::string("Error: cvh_multiphase_labels: ") + cvh_last_error(nullptr));
  if (!opt.dump_labels.empty()) write_raw_or_exit(opt.dump_labels, labels.data(), in.n);
  if (opt.select) {   // the label plane as a grey image: label x 85
    std::vector<uint8_t> grey(in.n);
    for (size_t q = 0; q < in.n; ++q) grey[q] = (uint8_t)(labels[q] * 85);
    write_or_exit(add_suffix(opt.input, "selection"), in.h, in.w, 1, grey.data());
  }
  if (opt.verbose) std::fprintf(stderr, "four phases: %d iterations, norms %.17g %.17g\n", steps, norms[0], norms[1]);
}

void run_two_phase(const Options &opt, Inputs &in, const cvh_params &prm)
{
  Run run(opt);
  make_run(run, opt, in, prm);
  cvh_context *ctx = run.ctx;
  // A coarse-to-fine run builds its start on the coarsest level, from planes that are restricted only after Perona-Malik: in iterate()
  if (opt.start.kind == Start::Rect && !opt.rect_ok) msg_exit("You must specify the contour with non-zero dimensions");
  if (opt.levels == 1) start_levelset(ctx, opt.start, opt, in);
  Frames frames(opt.input);   // the first frame before the channels are split / smoothed
  if (opt.video) {
    if (mkdir(frames.dir.c_str(), 0777) != 0 && errno != EEXIST) msg_exit("Error: cannot create \"" + frames.dir + "\"");
    if (opt.levels == 1) frames.write(ctx, opt, in, "t = 0");   // :930
  }
  if (opt.segment) {
    smooth_and_write_pm(run, opt, in);
    restart_from_image(run, opt, in);   // (the start above served the t = 0 frame)
  }
  // ---- colour space: behind Perona-Malik (<stem>_pm stays the picture the reference writes), in front of the iterations.  The loader's
  // planes are B, G, R.  Nothing is converted back: frames, _selection and _contour use the input image
  if (opt.colour_space) {
    cvh_check(run.ingest, cvh_convert_colour(run.ingest, opt.colour_space, CVH_ORDER_BGR, 0), "cvh_convert_colour");
    run.refresh_planes();
    restart_from_image(run, opt, in);
  }
  const Progress p = iterate(run, opt, in, frames);
  if (opt.energy) energy_line(ctx, opt.run_channels(), -1);
  if (!in.truth.empty()) print_score(ctx, opt, in);
  if (!opt.dump_planes.empty()) dump_planes(ctx, opt, in);
  if (!opt.dump_u.empty()) dump_levelset(ctx, opt, in);
  // --morph: the cleaned mask (-I applied as invert), morphed, becomes the level set on the device -- behind --dump-u, --energy and
  // --truth, which speak of the run's own level set; everything below then reads the result as a plain mask
  if (opt.split) {
    split_objects(ctx, opt, in);
    mask_outputs(ctx, opt, in, CleanArgs{opt.clean.conn, 0, 0, 0, 0}, false);
  } else if (opt.morph_op != CVH_MORPH_NONE) {
    cvh_check(ctx, with_clean(cvh_morph_levelset, ctx, opt.clean, opt.morph_op, opt.morph_r2, 1.0, -1.0), "cvh_morph_levelset");
    mask_outputs(ctx, opt, in, CleanArgs{opt.clean.conn, 0, 0, 0, 0}, false);
  } else {
    mask_outputs(ctx, opt, in, opt.clean, opt.clean_mask);
  }
  if (opt.verbose)  // the reference prints nothing
    std::fprintf(stderr, "chan_vese: %d iterations, last ||u_diff|| = %.17g\n", p.steps, p.norm);
  if (opt.verbose && opt.levels > 1) {
    std::fprintf(stderr, "chan_vese: iterations per level, finest first:");
    for (int s : p.level_steps) std::fprintf(stderr, " %d", s);
    std::fprintf(stderr, "\n");
  }
}

}  // namespace

int main(int argc, char **argv)
{
  const Options opt = read_options(parse_args(argc, argv));
  if (opt.help) { print_help(opt.verbose); return EXIT_SUCCESS; }
  Inputs in = load_inputs(opt);
  // ---- constants: src/main.cpp:890-895
  cvh_params prm;
  cvh_default_params(&prm);
  prm.mu = opt.mu; prm.nu = opt.nu; prm.dt = opt.dt; prm.eps = opt.eps; prm.tol = opt.tol;
  for (int k = 0; k < opt.run_channels(); ++k) { prm.lambda1[k] = opt.lambda1[k]; prm.lambda2[k] = opt.lambda2[k]; }
  if (opt.phases == 4) run_four_phase(opt, in, prm);
  else run_two_phase(opt, in, prm);
  return EXIT_SUCCESS;
}
