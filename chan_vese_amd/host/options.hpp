// options.hpp -- the command line of bin/chan_vese: the option table and the parser (the subset of boost::program_options behaviour the
// reference uses), the Options record with every value converted, read_options(), which fills it and issues every refusal that
// needs no image, in the reference's order with its messages (src/main.cpp:786-869) and this build's behind them, and print_help().
#pragma once
#include <cerrno>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <limits>
#include <string>
#include <vector>

#include "chanvese_hip.h"
#include "image_io.hpp"
#include "overlay_text.hpp"

// src/main.cpp:173-178
[[noreturn]] inline void msg_exit(const std::string &msg)
{
  std::cerr << "\n" << msg << "\n\n";
  std::exit(EXIT_FAILURE);
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
// what came after the table above and the --help text were pinned (tests/test_cli.py, tests/golden/cli_refusals.json): long names only,
// listed by --help --verbose
const Spec kLaterSpecs[] = {{"split", 0, 1}, {"split-labels", 0, 1}, {"edge", 0, 1}, {"dump-edge", 0, 1}, {"smooth", 0, 1}, {"smooth-sigma", 0, 1}, {"edge-sigma", 0, 1},
                            {"convex", 0, 1}, {"convex-means", 0, 1}, {"convex-stop", 0, 1}};

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

inline const Spec *find_long(const std::string &n)
{
  const Spec *hit = nullptr;
  int hits = 0;
  for (const Spec *table : {kSpecs, kLaterSpecs}) {
    const size_t rows = table == kSpecs ? sizeof(kSpecs) / sizeof(Spec) : sizeof(kLaterSpecs) / sizeof(Spec);
    for (size_t k = 0; k < rows; ++k) {
      const Spec &s = table[k];
      if (n == s.lname) return &s;
      if (std::string(s.lname).compare(0, n.size(), n) == 0) { hit = &s; ++hits; }  // unambiguous prefix
    }
  }
  return hits == 1 ? hit : nullptr;
}
inline const Spec *find_short(char c)
{
  for (const Spec &s : kSpecs) if (s.sname && s.sname == c) return &s;
  return nullptr;
}
inline bool looks_like_option(const std::string &t) { return t.size() >= 2 && t[0] == '-' && !std::isdigit((unsigned char)t[1]) && t[1] != '.'; }

inline Parsed parse_args(int argc, char **argv)
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

[[noreturn]] inline void invalid_argument(const std::string &opt, const std::string &v)
{
  msg_exit("error: the argument ('" + v + "') for option '--" + opt + "' is invalid");
}
inline double to_double(const std::string &opt, const std::string &v)
{
  char *end = nullptr;
  const double d = std::strtod(v.c_str(), &end);
  if (v.empty() || *end != '\0') invalid_argument(opt, v);
  return d;
}
inline long to_long(const std::string &opt, const std::string &v)
{
  char *end = nullptr;
  errno = 0;
  const long d = std::strtol(v.c_str(), &end, 10);
  if (v.empty() || *end != '\0' || errno == ERANGE) invalid_argument(opt, v);
  return d;
}
inline int to_int(const std::string &opt, const std::string &v)
{
  char *end = nullptr;
  const long d = std::strtol(v.c_str(), &end, 10);
  if (v.empty() || *end != '\0' || d > INT_MAX || d < INT_MIN) invalid_argument(opt, v);
  return (int)d;
}

// --local and --rank: a windowed filter by name, which stands for the code of every plane, and the radius of its window
// (--local-radius, --rank-radius), which one name (`bound`) may bind to less than radius_max
struct WindowName { const char *name; int code; };   // (a table ends with a null name)
struct WindowOption { const char *key, *label, *noun; const WindowName *names; int radius_max; const char *bound; int bound_max; };
const WindowName kLocalNames[] = {{"mean", CVH_LOCAL_MEAN}, {"dev", CVH_LOCAL_DEV}, {"stack", CVH_LOCAL_COPY}, {nullptr, 0}};   // (stack: read_options)
const WindowName kRankNames[] = {{"median", CVH_RANK_MEDIAN}, {"min", CVH_RANK_MIN}, {"max", CVH_RANK_MAX}, {"open", CVH_RANK_OPEN},
                                 {"close", CVH_RANK_CLOSE}, {"tophat", CVH_RANK_TOPHAT}, {"bothat", CVH_RANK_BOTHAT}, {nullptr, 0}};
const WindowOption kLocalOption = {"local", "Local", "statistic", kLocalNames, CVH_LOCAL_RADIUS_MAX, "", 0};
const WindowOption kRankOption = {"rank", "Rank", "filter", kRankNames, CVH_RANK_RADIUS_MAX, "median", CVH_RANK_MEDIAN_RADIUS_MAX};

// Whether the option is given; then every what[k] receives the code of `name` and `radius` is checked against the name's range.
// Refuses an unknown name and a radius without a name.
inline bool window_option(const Parsed &vm, const WindowOption &o, const std::string &name, int radius, int what[3])
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

// --line-color: ChanVese::Colors, src/main.cpp:111-118
struct LineColour { const char *name; uint8_t r, g, b; };
const LineColour kLineColours[] = {{"red", 255, 0, 0}, {"green", 0, 255, 0}, {"blue", 0, 0, 255}, {"black", 0, 0, 0},
                                   {"white", 255, 255, 255}, {"magenta", 255, 0, 255}, {"yellow", 255, 255, 0}, {"cyan", 0, 255, 255}};

// the mask the mask-based outputs speak of: what cvh_get_mask_clean and its kin take, in their order
struct CleanArgs { int conn, invert; long min_area, fill_holes; int largest; };

// how a level set starts; Rolled is the second level set's checkerboard of a four-phase run
struct Start {
  enum Kind { Checkerboard, Rect, Disk, Otsu, Threshold, Mask, Circ, Rolled } kind;
  int threshold;
  bool from_image() const { return kind == Otsu || kind == Threshold; }   // taken again when the planes change
};

struct Options {
  bool help = false;
  // the reference's options, defaults src/main.cpp:759-772
  std::string input;
  double mu = 0.5, nu = 0, dt = 1, eps = 1, tol = 0.001, fps = 10, K = 10, L = 0.25, T = 20;
  std::vector<double> lambda1, lambda2;
  int max_steps = -1;                              // as given; steps(): negative means unlimited
  overlay::Pos overlay_pos = overlay::Pos::TL;     // src/main.cpp:837-849
  uint8_t contour_bgr[3] = {255, 0, 0};            // blue
  bool segment = false, grayscale = false, video = false, overlay_text = false, select = false;
  // additions of this build
  std::string dump_u, dump_mask, dump_planes, dump_labels, measure, contours, truth, truth_labels, init_mask, split_labels, dump_edge;
  int device = 0, math_mode = CVH_MATH_FAST, state_bits = 64, reinit_every = 0, levels = 1, energy_every = 0, phases = 2, localized = 0;
  double edge = 0.0;   // --edge K: > 0 where given
  // --convex TAU[,SIGMA] with --convex-means M and --convex-stop S (chanvese_hip.h, "Convex relaxation"): cvh_convex_run in place of cvh_run
  bool convex = false;
  cvh_convex_params convex_params = {0.25, 0.5, 0.0, 1, 0, 0};
  // --smooth blur|detail with --smooth-sigma S, and --edge-sigma S: the taps are cvh_gauss_taps' (chanvese_hip.h, "Smoothing")
  bool smooth = false;
  double smooth_sigma = 1.0, edge_sigma = 0.0;   // edge_sigma > 0 where given
  int smooth_what[3] = {CVH_SMOOTH_COPY, CVH_SMOOTH_COPY, CVH_SMOOTH_COPY}, smooth_radius = 0, edge_radius = 0;
  uint16_t smooth_taps[CVH_SMOOTH_RADIUS_MAX + 1] = {0}, edge_taps[CVH_SMOOTH_RADIUS_MAX + 1] = {0};
  CleanArgs clean = {4, 0, 0, 0, 0};
  bool clean_mask = false;                         // a cleaning option is given: _selection, --dump-mask and --roi use the cleaned mask
  bool roi = false, energy = false, contours_all = false, contours_subpixel = false, verbose = false;
  Start start = {Start::Checkerboard, -1}, start2 = {Start::Rolled, -1};
  bool rect_ok = false, circ_ok = false;           // the numbers of --rect / --circ are refused only where they are used
  int rx = 0, ry = 0, rw = 0, rh = 0, cx = 0, cy = 0, cr = 0, disk_cx = 0, disk_cy = 0, disk_r = 0;
  bool local = false, rank = false, local_stack = false;
  int local_radius = 2, rank_radius = 1;
  int local_what[3] = {CVH_LOCAL_COPY, CVH_LOCAL_COPY, CVH_LOCAL_COPY}, rank_what[3] = {CVH_RANK_COPY, CVH_RANK_COPY, CVH_RANK_COPY};
  int colour_space = 0;                            // 0: the planes stay B, G, R
  int morph_op = CVH_MORPH_NONE;
  uint32_t morph_r2 = 1, score_tol2 = 4;           // floor(R^2) of --morph-radius and --score-tol
  bool split = false;                              // --split R: the stage split_objects (main.cpp) bakes the cut in front of the mask outputs
  uint32_t split_r2 = 0;                           // floor(R^2)
  bool one_plane = false;                          // the run has one plane: what the lambda counts and the threshold range follow

  int nof_channels() const { return grayscale ? 1 : 3; }   // planes read from the file
  int run_channels() const { return one_plane ? 1 : 3; }   // planes the run iterates on (--local stack: three of one)
  int steps() const { return max_steps < 0 ? std::numeric_limits<int>::max() : max_steps; }
};

// floor(x * x) as the uint32_t the library takes, capped at 2^32 - 1
inline uint32_t squared_capped(double x)
{
  const double s = std::floor(x * x);
  return s >= 4294967295.0 ? 0xffffffffu : (uint32_t)s;
}

// --lambda1 / --lambda2: src/main.cpp:800-829
inline void check_lambdas(const Parsed &vm, const std::string &name, bool one_plane, std::vector<double> &l)
{
  if (!vm.count(name)) { l.assign(one_plane ? 1 : 3, 1.0); return; }
  if (one_plane && l.size() != 1) msg_exit("Too many " + name + " values for a grayscale image.");
  else if (!one_plane && l.size() != 3) msg_exit("Number of " + name + " values must be 3 for a colored input image.");
  else if (one_plane && l[0] < 0) msg_exit("The value of " + name + " cannot be negative.");
  else if (!one_plane && (l[0] < 0 || l[1] < 0 || l[2] < 0)) msg_exit("Any value of " + name + " cannot be negative.");
}

// --threshold T and --init2 threshold T: the grey value is the sum of the planes
inline void check_threshold(int threshold, bool one_plane)
{
  const int top = 255 * (one_plane ? 1 : 3);
  if (threshold < 0 || threshold > top) msg_exit("Threshold must be between 0 and " + std::to_string(top) + ": " + std::to_string(threshold) + ".");
}

inline void refuse_combinations(const std::string &what, const std::vector<std::pair<bool, const char *>> &refused)
{
  for (auto &r : refused)
    if (r.first) msg_exit(what + " cannot be combined with " + r.second + ".");
}

// One value of one option into its variable, converted by the variable's type
struct ReadOne {
  const Parsed &vm;
  const std::string *one(const char *n) const { auto v = vm.get(n); return v && !v->empty() ? &(*v)[0] : nullptr; }
  void operator()(const char *n, std::string &dst) const { if (auto v = one(n)) dst = *v; }
  void operator()(const char *n, double &dst) const { if (auto v = one(n)) dst = to_double(n, *v); }
  void operator()(const char *n, int &dst) const { if (auto v = one(n)) dst = to_int(n, *v); }
  void operator()(const char *n, long &dst) const { if (auto v = one(n)) dst = to_long(n, *v); }
};

// Every option read and converted, then -- unless --help is given, which main() answers -- every refusal that needs no image.
inline Options read_options(const Parsed &vm)
{
  Options o;
  auto given = [&](const char *n) { return vm.count(n) > 0; };
  const ReadOne read{vm};
  std::string text_position = "TL", line_color = "blue", math = "fast", rect, circ, disk, init_kind = "checkerboard", colorspace, local_name,
              rank_name, morph_name, smooth_name, convex_steps;
  double morph_radius = 1.0, score_tol = 2.0, split_radius = 0.0;
  int threshold = -1;
  read("input", o.input);
  read("mu", o.mu);
  read("nu", o.nu);
  read("dt", o.dt);
  for (auto l : {std::make_pair("lambda1", &o.lambda1), std::make_pair("lambda2", &o.lambda2)})
    if (auto v = vm.get(l.first)) for (auto &s : *v) l.second->push_back(to_double(l.first, s));
  read("epsilon", o.eps);
  read("tolerance", o.tol);
  read("max-steps", o.max_steps);
  read("fps", o.fps);                      // (nothing to act on: -V writes an image sequence)
  read("overlay-pos", text_position);
  read("line-color", line_color);
  read("edge-coef", o.K);
  read("laplacian-coef", o.L);
  read("segment-time", o.T);
  read("dump-u", o.dump_u);
  read("dump-mask", o.dump_mask);
  read("device", o.device);
  read("math", math);
  read("state", o.state_bits);
  read("reinit", o.reinit_every);
  read("connectivity", o.clean.conn);
  read("min-area", o.clean.min_area);
  read("fill-holes", o.clean.fill_holes);
  read("morph", morph_name);
  read("morph-radius", morph_radius);
  read("init-mask", o.init_mask);
  read("rect", rect);
  read("circ", circ);
  read("disk", disk);
  read("init", init_kind);
  read("threshold", threshold);
  read("levels", o.levels);
  read("colorspace", colorspace);
  read("local", local_name);
  read("dump-planes", o.dump_planes);
  read("rank", rank_name);
  read("rank-radius", o.rank_radius);
  read("local-radius", o.local_radius);
  read("energy-every", o.energy_every);
  read("truth", o.truth);
  read("truth-labels", o.truth_labels);
  read("measure", o.measure);
  read("contours", o.contours);
  read("score-tol", score_tol);
  read("phases", o.phases);
  read("dump-labels", o.dump_labels);
  read("split", split_radius);
  read("split-labels", o.split_labels);
  o.split = given("split");
  read("localized", o.localized);   // --localized R (chanvese_hip.h, "Localised regions"): cvh_localized_run in place of cvh_run
  if (given("localized") && (o.localized < 1 || o.localized > 127))
    msg_exit("Window radius (--localized) must be between 1 and 127: " + std::to_string(o.localized) + ".");
  read("edge", o.edge);             // --edge K (chanvese_hip.h, "Edge-weighted length"): cvh_edge_map behind the Perona-Malik stage, cvh_geodesic_run in place of cvh_run
  read("dump-edge", o.dump_edge);
  if (given("edge") && (!(o.edge > 0.0) || !std::isfinite(o.edge)))
    msg_exit("Edge contrast (--edge) must be a finite number > 0: " + std::to_string(o.edge) + ".");
  read("smooth", smooth_name);      // --smooth blur|detail (chanvese_hip.h, "Smoothing"): cvh_smooth_planes behind --rank, in front of --local
  read("smooth-sigma", o.smooth_sigma);
  read("edge-sigma", o.edge_sigma);  // --edge-sigma S: the edge map of --edge is built from a blurred scratch copy of the planes
  read("convex", convex_steps);      // --convex TAU[,SIGMA]: the primal and the dual step; sigma defaults to 1 / (8 tau)
  read("convex-means", o.convex_params.means_every);
  read("convex-stop", o.convex_params.stop_rms);
  o.convex = given("convex");
  o.segment = given("segment"); o.grayscale = given("grayscale"); o.video = given("video"); o.overlay_text = given("overlay-text");
  o.select = given("select"); o.roi = given("roi"); o.energy = given("energy"); o.verbose = given("verbose");
  o.contours_all = given("contours-all"); o.contours_subpixel = given("contours-subpixel");
  o.clean.invert = given("invert-selection"); o.clean.largest = given("largest");
  o.clean_mask = given("connectivity") || given("min-area") || given("fill-holes") || o.clean.largest;
  o.help = given("help");
  if (o.help) return o;

  // ---- validation, in the reference's order with its messages: src/main.cpp:786-869
  if (!given("input")) msg_exit("Error: you have to specify input file name!");
  else if (!std::ifstream(o.input).good()) msg_exit("Error: file \"" + o.input + "\" does not exists!");
  if (o.dt <= 0) msg_exit("Cannot have negative or zero timestep: " + std::to_string(o.dt) + ".");
  if (o.mu < 0) msg_exit("Length penalty parameter cannot be negative: " + std::to_string(o.mu) + ".");
  // --local: the run iterates on local statistics of the planes (chanvese_hip.h, "Local statistics"); stack turns the grey plane into three
  o.local_stack = given("local") && iequals(local_name, "stack");
  if (o.local_stack && !o.grayscale) msg_exit("The local stack (--local stack) needs a grayscale read (-g): it makes three planes of one.");
  o.local = window_option(vm, kLocalOption, local_name, o.local_radius, o.local_what);
  if (o.local_stack) { o.local_what[1] = CVH_LOCAL_MEAN; o.local_what[2] = CVH_LOCAL_DEV; }
  // --rank: the run iterates on a rank filter of the planes (chanvese_hip.h, "Rank planes"), every plane alike
  o.rank = window_option(vm, kRankOption, rank_name, o.rank_radius, o.rank_what);
  // --smooth: the run iterates on the Gaussian blur of the planes or on what the blur leaves of them, every plane alike
  if (given("smooth-sigma") && !given("smooth")) msg_exit("A scale (--smooth-sigma) needs a smoothing (--smooth).");
  if (given("smooth")) {
    if (iequals(smooth_name, "blur")) o.smooth_what[0] = o.smooth_what[1] = o.smooth_what[2] = CVH_SMOOTH_BLUR;
    else if (iequals(smooth_name, "detail")) o.smooth_what[0] = o.smooth_what[1] = o.smooth_what[2] = CVH_SMOOTH_DETAIL;
    else msg_exit("Invalid smoothing requested.\nCorrect values are: blur, detail.");
    if (cvh_gauss_taps(o.smooth_sigma, o.smooth_taps, &o.smooth_radius) != CVH_OK)
      msg_exit("Smoothing scale (--smooth-sigma) must be a finite number > 0 and at most 21: " + std::to_string(o.smooth_sigma) + ".");
    o.smooth = true;
  }
  o.one_plane = o.grayscale && !o.local_stack;
  check_lambdas(vm, "lambda1", o.one_plane, o.lambda1);
  check_lambdas(vm, "lambda2", o.one_plane, o.lambda2);
  // (the reference's eps/tol checks look up non-existent keys and never fire: src/main.cpp:831-834)
  if (iequals(text_position, "TL")) o.overlay_pos = overlay::Pos::TL;
  else if (iequals(text_position, "BL")) o.overlay_pos = overlay::Pos::BL;
  else if (iequals(text_position, "TR")) o.overlay_pos = overlay::Pos::TR;
  else if (iequals(text_position, "BR")) o.overlay_pos = overlay::Pos::BR;
  else
    msg_exit("Invalid text position requested.\nCorrect values are: TL -- top left\n"
             "                    BL -- bottom left\n                    TR -- top right\n"
             "                    BR -- bottom right");
  {
    const LineColour *hit = nullptr;
    std::string list;
    for (const LineColour &c : kLineColours) {
      if (iequals(line_color, c.name)) hit = &c;
      list += std::string(list.empty() ? "" : ", ") + c.name;
    }
    if (!hit) msg_exit("Invalid contour color requested.\nCorrect values are: " + list + ".");
    o.contour_bgr[0] = hit->b; o.contour_bgr[1] = hit->g; o.contour_bgr[2] = hit->r;
  }
  if (o.L > 0.25 || o.L < 0) msg_exit("The Laplacian coefficient in Perona-Malik segmentation must be between 0 and 0.25.");
  if (given("segment-time") && o.T < o.L)
    msg_exit("The segmentation duration must exceed the value of Laplacian coefficient, " + std::to_string(o.L) + ".");
  if (given("rectangle") && given("circle")) msg_exit("Cannot initialize with both rectangular and circular contour");
  if (given("rectangle") || given("circle"))
    msg_exit("Interactive contour selection (-R/-C) needs a display and is not supported in this build; use --rect x,y,w,h or --circ cx,cy,r.");
  if (!rect.empty() && !circ.empty()) msg_exit("Cannot initialize with both rectangular and circular contour");
  if (init_kind != "checkerboard" && init_kind != "otsu") invalid_argument("init", init_kind);
  {
    const std::pair<bool, const char *> starts[] = {{!rect.empty(), "--rect"}, {!circ.empty(), "--circ"}, {!disk.empty(), "--disk"},
        {init_kind == "otsu", "--init otsu"}, {given("threshold"), "--threshold"}, {!o.init_mask.empty(), "--init-mask"}};
    const Start::Kind kinds[] = {Start::Rect, Start::Circ, Start::Disk, Start::Otsu, Start::Threshold, Start::Mask};
    std::vector<std::string> named;
    for (int k = 0; k < 6; ++k)
      if (starts[k].first) { named.push_back(starts[k].second); o.start = {kinds[k], threshold}; }
    if (named.size() > 1) msg_exit("Cannot initialize with both " + named[0] + " and " + named[1]);
  }
  o.rect_ok = std::sscanf(rect.c_str(), "%d,%d,%d,%d", &o.rx, &o.ry, &o.rw, &o.rh) == 4 && o.rw > 0 && o.rh > 0;
  o.circ_ok = std::sscanf(circ.c_str(), "%d,%d,%d", &o.cx, &o.cy, &o.cr) == 3 && o.cr > 0;  // is_ok(): radius > 0
  if (!disk.empty()) {
    char rest = 0;
    if (std::sscanf(disk.c_str(), "%d,%d,%d%c", &o.disk_cx, &o.disk_cy, &o.disk_r, &rest) != 3 || o.disk_r < 0)
      msg_exit("You must specify the disk as cx,cy,r with a radius that is not negative");
  }
  if (given("threshold")) check_threshold(threshold, o.one_plane);
  if (math != "strict" && math != "fast") invalid_argument("math", math);
  o.math_mode = math == "strict" ? CVH_MATH_STRICT : CVH_MATH_FAST;
  if (o.state_bits != 64 && o.state_bits != 32) invalid_argument("state", std::to_string(o.state_bits));
  if (o.reinit_every < 0) msg_exit("Reinitialisation interval cannot be negative: " + std::to_string(o.reinit_every) + ".");
  if (o.clean.conn != 4 && o.clean.conn != 8) msg_exit("Connectivity must be 4 or 8: " + std::to_string(o.clean.conn) + ".");
  if (o.clean.min_area < 0) msg_exit("Minimum component area cannot be negative: " + std::to_string(o.clean.min_area) + ".");
  if (o.clean.fill_holes < -1) msg_exit("Largest hole to fill must be -1 (any size), zero or positive: " + std::to_string(o.clean.fill_holes) + ".");
  if (o.reinit_every > 0 && o.video) msg_exit("Reinitialisation (--reinit) cannot be combined with video output (-V).");
  if (o.levels < 1) msg_exit("Number of levels must be at least 1: " + std::to_string(o.levels) + ".");
  if (o.levels > 1 && o.reinit_every > 0) msg_exit("Reinitialisation (--reinit) cannot be combined with a coarse-to-fine run (--levels).");
  if (o.levels > 1 && !circ.empty()) msg_exit("A circular outline (--circ) cannot be combined with a coarse-to-fine run (--levels); use --disk.");
  if (o.energy_every < 0) msg_exit("Energy interval cannot be negative: " + std::to_string(o.energy_every) + ".");
  if (!o.contours.empty() && o.video) msg_exit("A contour file (--contours) cannot be combined with video output (-V).");
  if (o.contours_all && o.contours.empty()) msg_exit("Every lattice vertex (--contours-all) needs a contour file (--contours).");
  if (o.contours_subpixel && o.contours.empty()) msg_exit("Subpixel points (--contours-subpixel) need a contour file (--contours).");
  if (o.contours_subpixel && o.contours_all) msg_exit("Subpixel points (--contours-subpixel) cannot be combined with every lattice vertex (--contours-all).");
  if (o.energy_every > 0 && o.video) msg_exit("An energy series (--energy-every) cannot be combined with video output (-V).");
  if (o.energy_every > 0 && o.reinit_every > 0) msg_exit("An energy series (--energy-every) cannot be combined with reinitialisation (--reinit).");
  if (o.energy_every > 0 && o.levels > 1) msg_exit("An energy series (--energy-every) cannot be combined with a coarse-to-fine run (--levels).");
  // --phases 4 (chanvese_hip.h, "Four phases"): two level sets, the second one started by --init2; what does not compose with it is refused
  if (o.phases != 2 && o.phases != 4) msg_exit("Number of phases must be 2 or 4: " + std::to_string(o.phases) + ".");
  if (auto v = vm.get("init2")) {
    if (o.phases != 4) msg_exit("A second start (--init2) needs four phases (--phases 4).");
    if (v->empty()) msg_exit("error: the required argument for option '--init2' is missing");
    const std::string &kind = (*v)[0];
    if (kind == "threshold") {
      if (v->size() != 2) msg_exit("A threshold start (--init2 threshold T) needs its threshold.");
      o.start2 = {Start::Threshold, to_int("init2", (*v)[1])};
      check_threshold(o.start2.threshold, o.one_plane);
    } else if ((kind != "checkerboard" && kind != "otsu") || v->size() != 1) {
      invalid_argument("init2", kind);
    } else if (kind == "otsu") {
      o.start2.kind = Start::Otsu;
    }
  }
  if (!o.dump_labels.empty() && o.phases != 4) msg_exit("A label file (--dump-labels) needs four phases (--phases 4).");
  if (o.phases == 4)
    refuse_combinations("Four phases (--phases 4)", {
        {o.video, "video output (-V)"}, {o.levels > 1, "a coarse-to-fine run (--levels)"}, {o.energy, "an energy line (--energy)"},
        {o.energy_every > 0, "an energy series (--energy-every)"}, {o.reinit_every > 0, "reinitialisation (--reinit)"},
        // the rest of what this build does not carry through two level sets: nothing is silently ignored
        {o.state_bits == 32, "FP32 state (--state 32)"}, {!rect.empty(), "--rect"}, {!circ.empty(), "--circ"}, {!disk.empty(), "--disk"},
        {!o.init_mask.empty(), "--init-mask"}, {given("local"), "--local"}, {given("rank"), "--rank"},
        {given("colorspace"), "--colorspace"}, {!o.dump_planes.empty(), "--dump-planes"}, {!o.dump_u.empty(), "--dump-u"},
        {!o.dump_mask.empty(), "--dump-mask"}, {o.clean_mask, "the cleaning options"}, {o.roi, "--roi"}, {given("morph"), "--morph"},
        {!o.truth.empty(), "--truth"}, {!o.truth_labels.empty(), "--truth-labels"}, {!o.measure.empty(), "--measure"},
        {!o.contours.empty(), "--contours"}, {o.clean.invert != 0, "an inverted selection (-I)"}, {o.split, "an object split (--split)"}, {given("smooth"), "--smooth"}});
  if (o.localized)
    refuse_combinations("Localised regions (--localized)", {
        {o.phases == 4, "four phases (--phases 4)"}, {o.levels > 1, "a coarse-to-fine run (--levels)"}, {o.energy, "an energy line (--energy)"},
        {o.energy_every > 0, "an energy series (--energy-every)"}, {o.reinit_every > 0, "reinitialisation (--reinit)"},
        {o.video, "video output (-V)"}, {o.state_bits == 32, "FP32 state (--state 32)"}});
  if (!o.dump_edge.empty() && !given("edge")) msg_exit("An edge map file (--dump-edge) needs an edge-weighted run (--edge).");
  if (given("edge-sigma") && !given("edge")) msg_exit("A blurred edge map (--edge-sigma) needs an edge-weighted run (--edge).");
  if (given("edge-sigma") && cvh_gauss_taps(o.edge_sigma, o.edge_taps, &o.edge_radius) != CVH_OK)
    msg_exit("Edge scale (--edge-sigma) must be a finite number > 0 and at most 21: " + std::to_string(o.edge_sigma) + ".");
  if (!given("edge-sigma")) o.edge_sigma = 0.0;
  if (given("edge"))
    refuse_combinations("Edge-weighted length (--edge)", {
        {o.phases == 4, "four phases (--phases 4)"}, {o.localized != 0, "localised regions (--localized)"}, {o.levels > 1, "a coarse-to-fine run (--levels)"},
        {o.energy, "an energy line (--energy)"}, {o.energy_every > 0, "an energy series (--energy-every)"},
        {o.reinit_every > 0, "reinitialisation (--reinit)"}, {o.video, "video output (-V)"}, {o.state_bits == 32, "FP32 state (--state 32)"}});
  // --convex (chanvese_hip.h, "Convex relaxation"): the relaxed model from the mask of the start; with --edge K the weighted model
  if ((given("convex-means") || given("convex-stop")) && !o.convex) msg_exit("The options --convex-means and --convex-stop need a convex run (--convex).");
  if (o.convex) {
    cvh_convex_params &q = o.convex_params;
    const size_t comma = convex_steps.find(',');
    q.tau = to_double("convex", convex_steps.substr(0, comma));
    q.sigma = comma == std::string::npos ? 1.0 / (8.0 * q.tau) : to_double("convex", convex_steps.substr(comma + 1));
    if (!(q.tau > 0.0) || !std::isfinite(q.tau) || !(q.sigma > 0.0) || !std::isfinite(q.sigma) || !(8.0 * q.tau * q.sigma <= 1.0))
      msg_exit("Convex steps (--convex TAU[,SIGMA]) must be finite numbers > 0 with 8 TAU SIGMA <= 1: " + convex_steps + ".");
    if (q.means_every < 0) msg_exit("Means interval (--convex-means) cannot be negative: " + std::to_string(q.means_every) + ".");
    if (std::isnan(q.stop_rms)) msg_exit("Stop level (--convex-stop) must be a number (negative: no stop rule).");
    q.use_edge = given("edge") ? 1 : 0;
    refuse_combinations("Convex relaxation (--convex)", {
        {o.phases == 4, "four phases (--phases 4)"}, {o.localized != 0, "localised regions (--localized)"}, {o.levels > 1, "a coarse-to-fine run (--levels)"},
        {o.energy, "an energy line (--energy)"}, {o.energy_every > 0, "an energy series (--energy-every)"},
        {o.reinit_every > 0, "reinitialisation (--reinit)"}, {o.video, "video output (-V)"}, {o.state_bits == 32, "FP32 state (--state 32)"}});
  }
  if (given("score-tol") && o.truth.empty()) msg_exit("A score tolerance (--score-tol) needs a ground truth (--truth).");
  if (!(score_tol >= 0.0) || !std::isfinite(score_tol)) msg_exit("Score tolerance must be a finite number >= 0.");
  o.score_tol2 = squared_capped(score_tol);
  if (given("morph")) {
    if (morph_name == "dilate") o.morph_op = CVH_MORPH_DILATE;
    else if (morph_name == "erode") o.morph_op = CVH_MORPH_ERODE;
    else if (morph_name == "open") o.morph_op = CVH_MORPH_OPEN;
    else if (morph_name == "close") o.morph_op = CVH_MORPH_CLOSE;
    else msg_exit("Invalid morphology requested.\nCorrect values are: dilate, erode, open, close.");
  }
  if (given("morph-radius") && !given("morph")) msg_exit("A radius (--morph-radius) needs an operation (--morph).");
  if (!(morph_radius >= 0.0) || !std::isfinite(morph_radius)) msg_exit("Morphology radius must be a finite number >= 0.");
  o.morph_r2 = squared_capped(morph_radius);
  // --split R (chanvese_hip.h, "Object split"): one level set, and the cleaned mask as it is -- a morphed mask is not split
  if (!o.split_labels.empty() && !o.split) msg_exit("A split label file (--split-labels) needs an object split (--split).");
  if (o.split && given("morph")) msg_exit("An object split (--split) cannot be combined with --morph.");
  if (!(split_radius >= 0.0) || !std::isfinite(split_radius)) msg_exit("Split radius must be a finite number >= 0.");
  o.split_r2 = squared_capped(split_radius);
  if (!o.init_mask.empty() && o.levels > 1)
    msg_exit("A mask start (--init-mask) cannot be combined with a coarse-to-fine run (--levels): a mask is not resampled.");
  if (!o.init_mask.empty() && !std::ifstream(o.init_mask).good())
    msg_exit("Error: file \"" + o.init_mask + "\" does not exists!");
  if (given("colorspace")) {
    if (iequals(colorspace, "ycrcb")) o.colour_space = CVH_COLOUR_YCRCB;
    else if (iequals(colorspace, "yuv")) o.colour_space = CVH_COLOUR_YUV;
    else msg_exit("Invalid colour space requested.\nCorrect values are: ycrcb, yuv.");
    if (o.grayscale) msg_exit("A colour space (--colorspace) cannot be combined with a grayscale read (-g): there is one plane.");
  }
  return o;
}

inline void print_help(bool later = false)
{
  const char *text =
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
  std::cout << text;
  // (the list above is pinned byte for byte by tests/golden/cli_refusals.json; what came later is listed by --help --verbose)
  if (!later) return;
  std::cout <<
      "Later additions:\n"
      "  --split arg                        R >= 0: take touching objects apart on the device -- the mask --dump-mask uses (cleaning options, -I)\n"
      "                                     is eroded by a disk of R pixels (dx^2 + dy^2 <= floor(R^2)), its cores grown back inside it, and a\n"
      "                                     one-pixel cut baked in where two objects meet; --dump-mask, --roi, --measure, --contours,\n"
      "                                     --truth-labels and _selection then see the split objects; not with --phases 4, --morph\n"
      "  --split-labels arg                 write the object labels of --split (cut pixels included, 0 = background, 1 .. K in raster order of\n"
      "                                     the cores) as raw little-endian int32 (h*w), the way --dump-u writes its raw plane\n"
      "  --edge arg                         K > 0: edge-weighted (geodesic) length term -- an edge map g = 1 / (1 + |grad I|^2 / K^2) is built on the\n"
      "                                     device from the planes the run iterates on, after the Perona-Malik stage (-S), and mu weighs g times the\n"
      "                                     contour length; honours --init / --rect / --circ / --disk / --init-mask; not with --phases 4, --localized,\n"
      "                                     --levels, --energy, --energy-every, --reinit, -V, --state 32\n"
      "  --dump-edge arg                    write the edge map of --edge as raw little-endian uint16 (h*w; 32768 = 1)\n"
      "  --smooth arg                       blur | detail: iterate on the Gaussian blur of every plane, or on 128 + plane - blur (the plane\n"
      "                                     without its smooth background); integer taps, replicated border; made on the device behind\n"
      "                                     Perona-Malik, --colorspace and --rank, in front of --local and the initial level set; not with --phases 4\n"
      "  --smooth-sigma arg (=1)            sigma of that Gaussian, 0 < sigma <= 21 (its radius is ceil(3 sigma))\n"
      "  --edge-sigma arg                   sigma, 0 < sigma <= 21: --edge builds its map from a Gaussian-blurred scratch copy of the planes,\n"
      "                                     g = 1 / (1 + |grad (G_sigma * I)|^2 / K^2), while the run iterates on the unblurred planes\n"
      "  --convex arg                       TAU[,SIGMA]: the convex relaxation of the two-phase model by primal-dual iterations from the mask of\n"
      "                                     the start -- for fixed means the result does not depend on it; the steps need 8 TAU SIGMA <= 1, SIGMA\n"
      "                                     defaults to 1 / (8 TAU); --mu, --nu, --lambda1, --lambda2 apply (scale the lambdas to about 1e-3), --dt,\n"
      "                                     -e and -t do not; honours --init / --rect / --circ / --disk / --init-mask / --threshold, and with\n"
      "                                     --edge K weighs the length by the edge map; the level set written is v - 1/2; not with --phases 4,\n"
      "                                     --localized, --levels, --energy, --energy-every, --reinit, -V, --state 32\n"
      "  --convex-means arg (=1)            retake the region means after every arg iterations (0: never after the start)\n"
      "  --convex-stop arg (=0)             stop once the root mean square of the update is at most arg (0: at an exact fixed point; negative:\n"
      "                                     never); -N stays the bound\n"
      "\n";
}
