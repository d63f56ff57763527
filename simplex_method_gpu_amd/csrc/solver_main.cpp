// solver_main.cpp — `./solver <file>` CLI, the drop-in for the reference's
// bin/solverN.out (main() at src/v4_cub_reduction.cu:384-473).
//
// Same argv, same LP text format (m n, A row-major, b, c; trailing text
// ignored — reader at v4:94-104, 401-419), same stdout: "# Iteration k" per
// loop pass (v4:136-142), the result block (v4:426-445) and the timing table
// (v4:456-471).  Compute goes through libsimplex's C-ABI only.
//
// Extra flags (all optional, before the file):
//   --max-iter K   loop passes (default: unlimited; reference MAX_ITER=5, v4:19)
//   --eps E        optimality tolerance (default 1e-7; reference 1e-4 f32, v4:18)
//   --compat       reference constants: --max-iter 5 --eps 1e-4
//   --gen m n seed solve the seeded random LP of SURVEY.md §8(d) (no file)
//   --device D     HIP device ordinal
//   --no-iter-lines  suppress the "# Iteration k" lines
//   --json         also print one JSON result line
//   --threads T    text-parser threads (default: min(16, cores))
//   --write-bin F  write the loaded/generated LP as binary .spxlp (lp_io.h)
//   --write-text F write it in the reference's text format (%.17g, exact)
//   --no-solve     stop after reading/writing
//   --ratio R      leaving-row rule: reference | guarded | harris (simplex.h
//                  SPX_RATIO_*; default reference, guarded with --mps)
//   --piv-tol T, --feas-tol T   tolerances of the guarded / Harris rules
//   --refactor K   rebuild B^-1 from the basis every K pivots (spx_reinvert)
//   --window W     B^-1 representation (0 auto, -1 explicit, 8..64 eta window)
//   --pricing P    entering-column rule: dantzig (v4:288-302, default) | devex | steepest
//   --dual         solve with the dual simplex loop (SPX_ALGO_DUAL, simplex.h): from
//                  the slack basis, which must be dual feasible (every c_j <= 0;
//                  b of any sign); "Problem infeasible." when no x >= 0 exists;
//                  a slack basis that is not dual feasible is an error (exit 1)
//   --dual-pricing R  leaving-row rule of --dual: dantzig (most negative x_b, default)
//                  | steepest (dual steepest edge, SPX_DUAL_PRICING_STEEPEST)
//   --dual-ratio R ratio test of --dual with --bounds: textbook (default) | long (the
//                  bound-flipping ratio test, SPX_DUAL_RATIO_LONG_STEP; --json
//                  then carries the flip counts).  --ratio stays the primal rule
//   --primal-box   solve with the bounded primal simplex loop (SPX_ALGO_PRIMAL_BOX,
//                  simplex.h): from the slack basis, which must be primal feasible
//                  (b >= 0, every bounded slack's u >= b_i); --json then carries
//                  the flip-pass and to-upper counts.  Not with --dual, --mps,
//                  --window N > 0 or --tableau (refused by name, exit 1)
//   --phase1       with --primal-box only (refused by name otherwise, exit 1): the
//                  loop's phase 1 (SPX_FLAG_PRIMAL_PHASE1), so the slack basis may
//                  be out of its bounds (b of any sign, any slack bounds); an
//                  infeasible LP ends with "Problem infeasible."; --json then
//                  also carries the phase-1 pass and pivot counts
//   --primal-pricing R  entering rule of --primal-box: dantzig (default) | steepest
//                  (exact steepest edge, SPX_PRIMAL_PRICING_STEEPEST); without
//                  --primal-box it is refused with the usage message (exit 1);
//                  not with --phase1 (the library's refusal is printed) unless
//                  --phase1-pricing steepest is given
//   --phase1-pricing R  entering rule of --phase1's passes under --primal-pricing
//                  steepest: dantzig (default: the combination is refused) |
//                  steepest (SPX_FLAG_PRIMAL_PHASE1_STEEPEST: phase 1 keys its
//                  candidates with the steepest-edge weights);
//                  inert without --phase1 or under --primal-pricing dantzig;
//                  without --primal-box it is refused by name (exit 1)
//   --phase1-ratio R  ratio test of --phase1's passes: textbook (default) | long
//                  (SPX_PRIMAL_RATIO_LONG_STEP, spx_set_primal_phase_one_ratio: the
//                  walk goes past rows that reach the bound they violate while
//                  the sum of violations still falls); with the
//                  option one more line "Long steps: rows passed R, passes P,
//                  most in one pass M" follows the result; inert without
//                  --phase1; an unknown word is refused by name (exit 1), and so
//                  is the option without --primal-box
//   --free-pricing R  entering rule of --primal-box where --lower holds a free
//                  column under --primal-pricing steepest: dantzig (default: the
//                  library's refusal is printed, exit 1) | steepest
//                  (SPX_FLAG_PRIMAL_FREE_STEEPEST: a free column is keyed with its
//                  steepest-edge weight); inert without a free
//                  column or under --primal-pricing dantzig; without --primal-box
//                  it is refused by name (exit 1)
//   --primal-weights W  how the steepest-edge weights of --primal-box restart
//                  for a warm basis: reference (default) | exact
//                  (SPX_FLAG_PRIMAL_EXACT_WEIGHTS); shown in --json.  The CLI
//                  starts from the slack basis, where both modes walk the same
//                  passes; an unknown word is refused by name (exit 1), and so
//                  is the option without --primal-box
//   --bounds F     upper bounds 0 <= x_j <= u_j of all n columns for --dual or
//                  --primal-box (spx_set_bounds): F holds n whitespace-separated
//                  values, "inf" = none; without either the library's refusal is
//                  printed (exit 1); not with --mps (its reader turns bounds into rows)
//   --lower F      lower bounds l_j <= x_j of all n columns for --dual or
//                  --primal-box (spx_set_bounds_lu), with or without --bounds: F
//                  in --bounds' format, "-inf" = a free column (--primal-box with
//                  Dantzig pricing, or steepest edge with --free-pricing steepest); z and x are in the caller's variables;
//                  without --dual or --primal-box it is refused by name (exit 1)
//   --ranging PREFIX  after a --dual or --primal-box solve that ends at the
//                  optimum: sensitivity ranging (spx_ranging_cost / _rhs, DESIGN.md
//                  §7k) written to PREFIX.cost.txt (one line per column: down up
//                  block_down block_up) and PREFIX.rhs.txt (one line per row: down
//                  up leave_down leave_up), "%.17g %.17g %lld %lld"; any other
//                  status prints the library's refusal (exit 1); without --dual or
//                  --primal-box it is refused by name (exit 1)
//   --bound-ranging PREFIX  after a --dual or --primal-box solve that ends at the
//                  optimum: bound ranging and the objective at the range ends
//                  (spx_ranging_bound / _objective) written to
//                  PREFIX.bound.txt (one line per column: down up leave_down
//                  leave_up obj_down obj_up), "%.17g %.17g %lld %lld %.17g %.17g";
//                  refusals as --ranging's
//   --tableau      window tableau (SPX_FLAG_TABLEAU): T_w = B_w A
//                  kept in HBM, no per-pivot A / B^-1 stream
//   --mps          the input is an MPS file (mps_io.h): converted to the
//                  canonical form (slacks, senses, bounds, big-M artificials)
//                  and solved; output as the reference's GLPK driver
//                  (solver_glpk.cpp:27-38: "x[i] = v" per original column,
//                  "Optimal objective: z", else "Problem status: <GLPK code>");
//                  --write-text then writes the converted LP (the fixed
//                  glpk_interface.cpp:80-98) with its recovery map as
//                  trailing comment lines
//   --big-m M      artificial cost (default 1e6 * max(1, max |c_j|))
// The input file may be text or binary; binary is detected by its magic.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iomanip>
#include <iostream>
#include <string>
#include <vector>

#include "../../include/simplex.h"
#include "lp_io.h"
#include "mps_io.h"

using Clock = std::chrono::steady_clock;
using TimePoint = Clock::time_point;

static double seconds(const TimePoint& a, const TimePoint& b) { return std::chrono::duration<double>(b - a).count(); }

static void print_elapsed_time(const char* msg, double dur) {
    auto label = std::string(msg) + ": ";
    std::cout << std::setw(19) << label;
    std::cout << std::fixed << std::setprecision(2);
    std::cout << std::setw(6) << dur << '\n';
}

static void usage() {
    std::cerr << "usage: solver [--max-iter K] [--eps E] [--compat] [--device D] [--no-iter-lines] [--json]"
                 " [--threads T] [--write-bin F] [--write-text F] [--no-solve] [--ratio reference|guarded|harris]"
                 " [--piv-tol T] [--feas-tol T] [--refactor K] [--window W] [--pricing dantzig|devex|steepest] [--tableau] [--dual] [--primal-box [--phase1] [--primal-pricing dantzig|steepest] [--phase1-pricing dantzig|steepest] [--free-pricing dantzig|steepest] [--primal-weights reference|exact]]"
                 " [--dual-pricing dantzig|steepest] [--dual-ratio textbook|long] [--bounds F] [--lower F] [--ranging PREFIX] [--bound-ranging PREFIX] [--phase1-ratio textbook|long]"
                 " [--mps [--big-m M]]"
                 " (<file> | --gen m n seed)\n";
}

int main(int argc, char* argv[]) {
    std::ios_base::sync_with_stdio(false);
    int64_t max_iter = INT64_MAX;
    double eps = 1e-7;
    int device = -1;
    bool iter_lines = true, json = false, gen = false, solve = true;
    int threads = 0;
    std::string write_bin, write_text, bounds_path, lower_path, ranging_prefix, bound_ranging_prefix;
    int64_t gm = 0, gn = 0;
    uint64_t gseed = 0;
    const char* path = nullptr;
    int ratio = -1, window = 0, pricing = SPX_PRICING_DANTZIG;
    double piv_tol = 1e-9, feas_tol = 1e-9, big_m = 0.0;
    int64_t refactor = 0;
    bool mps_in = false, tableau = false, dual = false, dual_steepest = false, dual_long = false, primal_box = false, phase1 = false;
    bool primal_pricing_given = false, primal_steepest = false;
    bool primal_weights_given = false, primal_exact = false;
    bool phase1_pricing_given = false, phase1_steepest = false;
    bool phase1_ratio_given = false, phase1_long = false;
    bool free_pricing_given = false, free_steepest = false;
    for (int a = 1; a < argc; ++a) {
        const std::string s = argv[a];
        auto need = [&](int k) {
            if (a + k >= argc) {
                usage();
                std::exit(1);
            }
        };
        if (s == "--max-iter") { need(1); max_iter = std::strtoll(argv[++a], nullptr, 10); }
        else if (s == "--eps") { need(1); eps = std::strtod(argv[++a], nullptr); }
        else if (s == "--compat") { max_iter = 5; eps = 1e-4; }
        else if (s == "--device") { need(1); device = std::atoi(argv[++a]); }
        else if (s == "--no-iter-lines") iter_lines = false;
        else if (s == "--json") json = true;
        else if (s == "--threads") { need(1); threads = std::atoi(argv[++a]); }
        else if (s == "--write-bin") { need(1); write_bin = argv[++a]; }
        else if (s == "--write-text") { need(1); write_text = argv[++a]; }
        else if (s == "--no-solve") solve = false;
        else if (s == "--ratio") {
            need(1);
            const std::string r = argv[++a];
            ratio = r == "reference" ? SPX_RATIO_REFERENCE
                  : r == "guarded"   ? SPX_RATIO_GUARDED
                  : r == "harris"    ? SPX_RATIO_HARRIS
                                     : -2;
            if (ratio == -2) { usage(); return 1; }
        }
        else if (s == "--piv-tol") { need(1); piv_tol = std::strtod(argv[++a], nullptr); }
        else if (s == "--feas-tol") { need(1); feas_tol = std::strtod(argv[++a], nullptr); }
        else if (s == "--refactor") { need(1); refactor = std::strtoll(argv[++a], nullptr, 10); }
        else if (s == "--window") { need(1); window = std::atoi(argv[++a]); }
        else if (s == "--mps") mps_in = true;
        else if (s == "--tableau") tableau = true;
        else if (s == "--dual") dual = true;
        else if (s == "--primal-box") primal_box = true;
        else if (s == "--phase1") phase1 = true;
        else if (s == "--ranging") { need(1); ranging_prefix = argv[++a]; }
        else if (s == "--bound-ranging") { need(1); bound_ranging_prefix = argv[++a]; }
        else if (s == "--bounds") { need(1); bounds_path = argv[++a]; }
        else if (s == "--lower") { need(1); lower_path = argv[++a]; }
        else if (s == "--dual-pricing") {
            need(1);
            const std::string r = argv[++a];
            if (r != "dantzig" && r != "steepest") { usage(); return 1; }
            dual_steepest = r == "steepest";
        }
        else if (s == "--primal-pricing") {
            need(1);
            const std::string r = argv[++a];
            if (r != "dantzig" && r != "steepest") { usage(); return 1; }
            primal_pricing_given = true;
            primal_steepest = r == "steepest";
        }
        else if (s == "--phase1-pricing") {
            need(1);
            const std::string r = argv[++a];
            if (r != "dantzig" && r != "steepest") {
                std::cerr << "--phase1-pricing " << r << ": dantzig or steepest\n";
                return 1;
            }
            phase1_pricing_given = true;
            phase1_steepest = r == "steepest";
        }
        else if (s == "--phase1-ratio") {
            need(1);
            const std::string r = argv[++a];
            if (r != "textbook" && r != "long") {
                std::cerr << "--phase1-ratio " << r << ": textbook or long\n";
                return 1;
            }
            phase1_ratio_given = true;
            phase1_long = r == "long";
        }
        else if (s == "--free-pricing") {
            need(1);
            const std::string r = argv[++a];
            if (r != "dantzig" && r != "steepest") {
                std::cerr << "--free-pricing " << r << ": dantzig or steepest\n";
                return 1;
            }
            free_pricing_given = true;
            free_steepest = r == "steepest";
        }
        else if (s == "--primal-weights") {
            need(1);
            const std::string r = argv[++a];
            if (r != "reference" && r != "exact") {
                std::cerr << "--primal-weights " << r << ": reference or exact\n";
                return 1;
            }
            primal_weights_given = true;
            primal_exact = r == "exact";
        }
        else if (s == "--dual-ratio") {
            need(1);
            const std::string r = argv[++a];
            if (r != "textbook" && r != "long") { usage(); return 1; }
            dual_long = r == "long";
        }
        else if (s == "--pricing") {
            need(1);
            const std::string r = argv[++a];
            pricing = r == "dantzig" ? SPX_PRICING_DANTZIG
                      : r == "devex"   ? SPX_PRICING_DEVEX
                      : r == "steepest" ? SPX_PRICING_STEEPEST
                                        : -1;
            if (pricing < 0) { usage(); return 1; }
        }
        else if (s == "--big-m") { need(1); big_m = std::strtod(argv[++a], nullptr); }
        else if (s == "--gen") {
            need(3);
            gen = true;
            gm = std::strtoll(argv[++a], nullptr, 10);
            gn = std::strtoll(argv[++a], nullptr, 10);
            gseed = std::strtoull(argv[++a], nullptr, 10);
        } else if (s == "-h" || s == "--help") { usage(); return 0; }
        else if (!path) path = argv[a];
        else { usage(); return 1; }
    }
    if (!path && !gen) {
        std::cerr << "Please, specify an input file.\n";
        return 1;
    }
    if (phase1 && !primal_box) {
        std::cerr << "--phase1 needs --primal-box: it is the bounded primal loop's phase 1\n";
        return 1;
    }
    if (!lower_path.empty() && !primal_box && !dual) {
        std::cerr << "--lower needs --dual or --primal-box: lower bounds are the bounded loops'\n";
        return 1;
    }
    if (!ranging_prefix.empty() && !primal_box && !dual) {
        std::cerr << "--ranging needs --dual or --primal-box: ranging describes an optimum of the bounded loops\n";
        return 1;
    }
    if (!bound_ranging_prefix.empty() && !primal_box && !dual) {
        std::cerr << "--bound-ranging needs --dual or --primal-box: ranging describes an optimum of the bounded loops\n";
        return 1;
    }
    if (primal_pricing_given && !primal_box) {
        std::cerr << "--primal-pricing needs --primal-box: it is the bounded primal loop's entering rule\n";
        usage();
        return 1;
    }
    if (phase1_pricing_given && !primal_box) {
        std::cerr << "--phase1-pricing needs --primal-box: it is the rule of the bounded primal loop's phase 1\n";
        return 1;
    }
    if (phase1_ratio_given && !primal_box) {
        std::cerr << "--phase1-ratio needs --primal-box: it is the ratio test of the bounded primal loop's phase 1\n";
        return 1;
    }
    if (free_pricing_given && !primal_box) {
        std::cerr << "--free-pricing needs --primal-box: it is the bounded primal loop's rule with free columns\n";
        return 1;
    }
    if (primal_weights_given && !primal_box) {
        std::cerr << "--primal-weights needs --primal-box: it is the bounded primal loop's weight start\n";
        return 1;
    }
    if (primal_box) {
        const char* with = dual ? "--dual" : mps_in ? "--mps" : window > 0 ? "--window N > 0" : tableau ? "--tableau" : nullptr;
        if (with) {
            std::cerr << "--primal-box does not combine with " << with << "\n";
            return 1;
        }
    }

    const TimePoint t_start = Clock::now();
    TimePoint t_host_alloc = t_start, t_read = t_start, t_solve = t_start;
    lpio::LP lp;
    mps::Problem pb;
    std::string err, trailer;
    if (mps_in && !gen) {
        t_host_alloc = t_read = Clock::now();
        if (mps::read_mps(path, pb, err, big_m) != 0) {
            std::cerr << err << "\n";
            return EXIT_FAILURE;
        }
        lp = std::move(pb.lp);
        trailer = mps::map_block(pb);
    } else if (!gen) {
        t_host_alloc = t_read = Clock::now();
        if (lpio::read_any(path, lp, err, threads) != 0) {
            std::cerr << err << "\n";
            return EXIT_FAILURE;
        }
    } else {
        lp.m = gm;
        lp.n = gn;
        t_host_alloc = t_read = Clock::now();
        if (!write_bin.empty() || !write_text.empty()) lpio::generate(gm, gn, gseed, lp);
    }
    if ((!write_bin.empty() && lpio::write_binary(write_bin, lp, err) != 0) ||
        (!write_text.empty() && lpio::write_text(write_text, lp, err, trailer) != 0)) {
        std::cerr << err << "\n";
        return EXIT_FAILURE;
    }
    if (!solve) return 0;
    const int64_t m = lp.m, n = lp.n;
    const bool device_gen = gen && lp.A.empty();
    std::vector<double> x_b((size_t)std::max<int64_t>(m, 1));
    std::vector<int64_t> b_ixs((size_t)std::max<int64_t>(m, 1));

    t_solve = Clock::now();
    spx_opts o;
    spx_default_opts(&o);
    o.eps = eps;
    o.device = device;
    o.ratio_test = ratio >= 0 ? ratio : (mps_in ? SPX_RATIO_GUARDED : SPX_RATIO_REFERENCE);
    o.piv_tol = piv_tol;
    o.feas_tol = feas_tol;
    o.refactor_every = (int32_t)refactor;
    o.window = window;
    o.pricing = pricing;
    if (tableau) o.flags |= SPX_FLAG_TABLEAU;
    if (dual) o.algorithm = SPX_ALGO_DUAL;
    if (primal_box) o.algorithm = SPX_ALGO_PRIMAL_BOX;
    if (dual_steepest) o.flags |= SPX_FLAG_DUAL_STEEPEST;
    if (dual_long) o.flags |= SPX_FLAG_DUAL_LONG_STEP;
    if (phase1) o.flags |= SPX_FLAG_PRIMAL_PHASE1;
    if (primal_steepest) o.flags |= SPX_FLAG_PRIMAL_STEEPEST;
    if (primal_exact) o.flags |= SPX_FLAG_PRIMAL_EXACT_WEIGHTS;
    if (phase1_steepest) o.flags |= SPX_FLAG_PRIMAL_PHASE1_STEEPEST;
    if (free_steepest) o.flags |= SPX_FLAG_PRIMAL_FREE_STEEPEST;
    spx_ctx* ctx = nullptr;
    const TimePoint t_alloc = Clock::now();
    int rc = device_gen ? spx_create_generated(&ctx, m, n, gseed, &o)
                        : spx_create(&ctx, m, n, lp.A.data(), lp.b.data(), lp.c.data(), &o);
    if (rc != SPX_OK) {
        std::cerr << "spx_create failed (" << rc << "): " << spx_last_error() << "\n";
        return EXIT_FAILURE;
    }
    if (!bounds_path.empty() || !lower_path.empty()) {
        const char* opt = !bounds_path.empty() ? "--bounds" : "--lower";
        if (mps_in) {
            std::cerr << opt << " does not combine with --mps: the MPS reader turns bounds into rows\n";
            spx_destroy(ctx);
            return EXIT_FAILURE;
        }
        // n whitespace-separated values ("inf" / "+inf" / "-inf" / "infinity" parse as infinities)
        auto read_values = [&](const char* name, const std::string& file, const char* none, std::vector<double>& out) {
            std::ifstream bf(file);
            std::string tok;
            bool bad = !bf;
            while (!bad && bf >> tok) {
                char* end = nullptr;
                const double v = std::strtod(tok.c_str(), &end);
                if (end == tok.c_str() || *end != '\0') bad = true;
                out.push_back(v);
            }
            if (bad || (int64_t)out.size() != n) {
                std::cerr << name << " " << file << ": expected " << n << " values (one per column, " << none << ")\n";
                return false;
            }
            return true;
        };
        std::vector<double> ub, lb;
        if ((!bounds_path.empty() && !read_values("--bounds", bounds_path, "inf = none", ub)) ||
            (!lower_path.empty() && !read_values("--lower", lower_path, "-inf = free", lb))) {
            spx_destroy(ctx);
            return EXIT_FAILURE;
        }
        const char* call = lb.empty() ? "spx_set_bounds" : "spx_set_bounds_lu";
        rc = lb.empty() ? spx_set_bounds(ctx, ub.data()) : spx_set_bounds_lu(ctx, lb.data(), ub.empty() ? nullptr : ub.data());
        if (rc != SPX_OK) {
            std::cerr << call << " failed (" << rc << "): " << spx_last_error() << "\n";
            spx_destroy(ctx);
            return EXIT_FAILURE;
        }
    }
    if (phase1_long) {
        rc = spx_set_primal_phase_one_ratio(ctx, SPX_PRIMAL_RATIO_LONG_STEP);
        if (rc != SPX_OK) {
            std::cerr << "spx_set_primal_phase_one_ratio failed (" << rc << "): " << spx_last_error() << "\n";
            spx_destroy(ctx);
            return EXIT_FAILURE;
        }
    }
    const TimePoint t_init_end = Clock::now();
    double z = 0.0;
    int32_t status = 0;
    int64_t pivots = 0;
    rc = spx_solve(ctx, max_iter, &z, b_ixs.data(), x_b.data(), &status, &pivots);
    if (rc != SPX_OK) {
        std::cerr << "spx_solve failed (" << rc << "): " << spx_last_error() << "\n";
        spx_destroy(ctx);
        return EXIT_FAILURE;
    }
    const TimePoint t_loop_end = Clock::now();
    int64_t flips[3] = {0, 0, 0};
    if (dual) spx_get_dual_flips(ctx, flips);
    int64_t pflips[2] = {0, 0};
    if (primal_box) spx_get_primal_flips(ctx, pflips);
    int64_t ph1[4] = {0, 0, 0, 0};
    if (phase1) spx_get_primal_phase1(ctx, ph1);
    int64_t lsteps[4] = {0, 0, 0, 0};
    if (phase1_ratio_given) spx_get_primal_long_steps(ctx, lsteps);
    if (!ranging_prefix.empty()) {  // PREFIX.cost.txt (n lines) and PREFIX.rhs.txt (m lines): down up index index
        std::vector<double> dn((size_t)n), up((size_t)n);
        std::vector<int64_t> kd((size_t)n), ku((size_t)n);
        auto write = [&](const std::string& file, int64_t count) {
            std::FILE* f = std::fopen(file.c_str(), "w");
            if (!f) {
                std::cerr << "--ranging: cannot write " << file << "\n";
                return false;
            }
            for (int64_t k = 0; k < count; ++k)
                std::fprintf(f, "%.17g %.17g %lld %lld\n", dn[(size_t)k], up[(size_t)k], (long long)kd[(size_t)k],
                             (long long)ku[(size_t)k]);
            return std::fclose(f) == 0;
        };
        rc = spx_ranging_cost(ctx, dn.data(), up.data(), kd.data(), ku.data());
        bool ok = rc == SPX_OK && write(ranging_prefix + ".cost.txt", n);
        if (ok) {
            rc = spx_ranging_rhs(ctx, dn.data(), up.data(), kd.data(), ku.data());
            ok = rc == SPX_OK && write(ranging_prefix + ".rhs.txt", m);
        }
        if (!ok) {
            if (rc != SPX_OK) std::cerr << "--ranging failed (" << rc << "): " << spx_last_error() << "\n";
            spx_destroy(ctx);
            return EXIT_FAILURE;
        }
    }
    if (!bound_ranging_prefix.empty()) {  // PREFIX.bound.txt (n lines): down up index index obj_down obj_up
        std::vector<double> dn((size_t)n), up((size_t)n), zd((size_t)n), zu((size_t)n);
        std::vector<int64_t> kd((size_t)n), ku((size_t)n);
        rc = spx_ranging_bound(ctx, dn.data(), up.data(), kd.data(), ku.data());
        if (rc == SPX_OK) rc = spx_ranging_objective(ctx, SPX_RANGING_BOUND, dn.data(), up.data(), zd.data(), zu.data());
        if (rc != SPX_OK) {
            std::cerr << "--bound-ranging failed (" << rc << "): " << spx_last_error() << "\n";
            spx_destroy(ctx);
            return EXIT_FAILURE;
        }
        const std::string file = bound_ranging_prefix + ".bound.txt";
        std::FILE* f = std::fopen(file.c_str(), "w");
        if (f)
            for (int64_t k = 0; k < n; ++k)
                std::fprintf(f, "%.17g %.17g %lld %lld %.17g %.17g\n", dn[(size_t)k], up[(size_t)k],
                             (long long)kd[(size_t)k], (long long)ku[(size_t)k], zd[(size_t)k], zu[(size_t)k]);
        if (!f || std::fclose(f) != 0) {
            std::cerr << "--bound-ranging: cannot write " << file << "\n";
            spx_destroy(ctx);
            return EXIT_FAILURE;
        }
    }
    spx_destroy(ctx);
    const TimePoint t_dealloc_end = Clock::now();

    if (mps_in) {  // the reference's GLPK driver output (solver_glpk.cpp:27-38)
        pb.lp.m = m;
        pb.lp.n = n;
        std::vector<double> xb(x_b.begin(), x_b.begin() + m);
        std::vector<int64_t> bix(b_ixs.begin(), b_ixs.begin() + m);
        const double art = mps::max_artificial(pb, xb, bix);
        double bmax = 1.0;
        for (double v : lp.b) bmax = std::max(bmax, std::fabs(v));
        const bool feasible = art <= 1e-7 * bmax;
        const std::vector<double> xs = mps::recover_x(pb, xb, bix);
        const double zo = mps::objective(pb, xs);
        // GLPK status codes: GLP_OPT 5, GLP_NOFEAS 4, GLP_UNBND 6, GLP_UNDEF 1
        const int glp = status == SPX_STATUS_OPTIMUM_FOUND ? (feasible ? 5 : 4)
                        : status == SPX_STATUS_UNBOUNDED   ? 6
                                                           : 1;
        if (glp == 5) {
            for (size_t j = 0; j < xs.size(); ++j) std::cout << "x[" << j + 1 << "] = " << xs[j] << "\n";
            std::cout << "Optimal objective: " << zo << "\n";
        } else {
            std::cout << "Problem status: " << glp << "\n";
        }
        if (json) {
            std::cout << std::defaultfloat << std::setprecision(17);
            std::cout << "{\"status\": " << status << ", \"glp_status\": " << glp << ", \"z\": " << zo
                      << ", \"pivots\": " << pivots << ", \"m\": " << m << ", \"n\": " << n
                      << ", \"max_artificial\": " << art << ", \"x\": [";
            for (size_t j = 0; j < xs.size(); ++j) std::cout << (j ? ", " : "") << xs[j];
            std::cout << "]}\n";
        }
        return 0;
    }

    // "# Iteration k" once per loop pass (v4:287): pivots + the terminating pass
    const int64_t passes = (status == SPX_STATUS_MAX_ITER) ? pivots : pivots + 1;
    if (iter_lines)
        for (int64_t i = 1; i <= passes; ++i) std::cout << "# Iteration " << i << '\n';

    const TimePoint t_print = Clock::now();
    switch (status) {
        case SPX_STATUS_OPTIMUM_FOUND:
            std::cout << "Optimum found: " << z << '\n';
            for (int64_t i = 0; i < m; ++i) std::cout << "\tx_" << b_ixs[(size_t)i] << " = " << x_b[(size_t)i] << "\n";
            break;
        case SPX_STATUS_UNBOUNDED: std::cout << "Problem unbounded.\n"; break;
        case SPX_STATUS_THETA_OVERFLOW: std::cout << "Theta overflow.\n"; break;
        case SPX_STATUS_INFEASIBLE: std::cout << "Problem infeasible.\n"; break;
        default: std::cout << "MAX_ITER exceeded.\n"; break;
    }
    if (phase1_ratio_given)
        std::cout << "Long steps: rows passed " << lsteps[0] << ", passes " << lsteps[1] << ", most in one pass "
                  << lsteps[2] << '\n';
    std::cout << '\n';
    const TimePoint t_host_free = Clock::now();
    lp = lpio::LP();
    const TimePoint t_end = Clock::now();

    // timing table (v4:456-471).  The reference's y / x_b phases are fused into
    // the update kernel here, so the whole device loop is reported under p and
    // B_inv is 0 (per-kernel device times: bench.py / spx_kernel_times).
    print_elapsed_time("Total", seconds(t_start, t_end));
    std::cout << '\n';
    print_elapsed_time("y", 0.0);
    print_elapsed_time("p", seconds(t_init_end, t_loop_end));
    print_elapsed_time("B_inv", 0.0);
    print_elapsed_time("x_b", 0.0);
    std::cout << '\n';
    print_elapsed_time("Alloc", seconds(t_alloc, t_init_end));
    print_elapsed_time("Init", 0.0);
    print_elapsed_time("Dealloc", seconds(t_loop_end, t_dealloc_end));
    std::cout << '\n';
    print_elapsed_time("Host alloc", seconds(t_host_alloc, t_read));
    print_elapsed_time("Read file", seconds(t_read, t_solve));
    print_elapsed_time("Solve call", seconds(t_solve, t_print));
    print_elapsed_time("Print result", seconds(t_print, t_host_free));
    print_elapsed_time("Host free", seconds(t_host_free, t_end));

    if (json) {
        std::cout << std::defaultfloat << std::setprecision(17);
        std::cout << "{\"status\": " << status << ", \"z\": " << z << ", \"pivots\": " << pivots
                  << ", \"m\": " << m << ", \"n\": " << n;
        if (dual)
            std::cout << ", \"dual_ratio\": \"" << (dual_long ? "long" : "textbook") << "\", \"flips\": " << flips[0]
                      << ", \"flip_passes\": " << flips[1] << ", \"max_flips\": " << flips[2];
        if (primal_box)
            std::cout << ", \"flip_passes\": " << pflips[0] << ", \"to_upper\": " << pflips[1]
                      << ", \"primal_weights\": \"" << (primal_exact ? "exact" : "reference") << "\"";
        if (phase1)
            std::cout << ", \"phase1_passes\": " << ph1[0] << ", \"phase1_pivots\": " << ph1[1]
                      << ", \"phase1_rows\": " << ph1[2];
        std::cout << ", \"solve_s\": " << seconds(t_init_end, t_loop_end) << "}\n";
    }
    return 0;
}
