// Stand-alone check of lb::speculative_lattice (bioen_amd/csrc/lbfgs_state.hpp) against the state machine it foresees:
// compiled with g++ from that header alone and run by tests/test_spec_lattice.py.
//
// The machine is driven through scripted line searches (every trial result is made up so that the search takes the
// scripted move).  Before every trial the generator is asked for its list; after every rejection the step the machine
// asks for must be, bit for bit, the member of EVERY list issued earlier in that search at the position the order rules
// give -- restated here independently of the generator:
//   linesearch 1:      [d, dd, ddd, ...]                                    (the chain of halvings, kLatticeDepth deep)
//   linesearch 2, 3:   [d, u, chain 2, ..., chain kLatticeDepth, the second-level nodes the chain has not got: dd, uu, du]
//   chain: the move the search is expected to make next, and so on -- a run goes on, two different moves alternate,
//   no move yet: down, except in the first search of a problem (iteration 0): up.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../bioen_amd/csrc/lbfgs_state.hpp"

using namespace bioen;

static int failures = 0;
static long checks = 0;

#define CHECK(cond, ...)                                  \
    do {                                                  \
        ++checks;                                         \
        if (!(cond)) {                                    \
            ++failures;                                   \
            std::printf("FAIL line %d: ", __LINE__);      \
            std::printf(__VA_ARGS__);                     \
            std::printf("\n");                            \
        }                                                 \
    } while (0)

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

// the order rules, restated -----------------------------------------------------------------------------------------
static int habit(int ls, int last, int prev, int iteration) {
    if (ls == 1) return -1;
    if (last == 0) return iteration == 0 ? +1 : -1;
    if (prev != 0 && prev != last) return -last;
    return last;
}

// where in a list issued with (ls, last, prev, iteration) the step reached by `moves` must sit; -1: not promised
static int expected_index(int ls, int last, int prev, int iteration, const std::vector<int>& moves) {
    const int t = (int)moves.size();
    if (t == 1) return ls == 1 ? 0 : (moves[0] < 0 ? 0 : 1);
    std::vector<int> pred;
    int h1 = last, h2 = prev;
    for (int i = 0; i < lb::kLatticeDepth; ++i) {
        const int mv = habit(ls, h1, h2, iteration);
        pred.push_back(mv);
        h2 = h1;
        h1 = mv;
    }
    bool on_chain = t <= lb::kLatticeDepth;
    for (int i = 0; i < t && on_chain; ++i) on_chain = moves[i] == pred[i];
    if (on_chain) return ls == 1 ? t - 1 : t;            // [d, u, chain 2, chain 3, ...]: chain t at index t
    if (t == 2 && ls != 1) {
        auto node = [](int a, int b) { return a == b ? (a < 0 ? 0 : 1) : 2; };      // dd, uu, du
        const int mine = node(moves[0], moves[1]), chain2 = node(pred[0], pred[1]);
        int rank = 0;
        for (int kind = 0; kind < mine; ++kind) rank += kind != chain2;
        return 2 + (lb::kLatticeDepth - 1) + rank;
    }
    return -1;
}

struct Issued {
    double out[lb::kLatticeMax];
    int n, last, prev, iteration;
    std::vector<int> moves;       // the search's moves since
};

static void check_list(const double* out, int n, int capacity, const char* what) {
    CHECK(n <= capacity && n <= lb::kLatticeMax, "%s: %d steps for capacity %d", what, n, capacity);
    for (int i = 0; i < n; ++i) {
        CHECK(kMinStep <= out[i] && out[i] <= kMaxStep, "%s: step %d = %g out of bounds", what, i, out[i]);
        for (int j = 0; j < i; ++j) CHECK(!same_bits(out[i], out[j]), "%s: steps %d and %d are the same", what, j, i);
    }
}

// One problem: `searches` are strings of moves ('d' decrease test fails, 'D' strong-Wolfe test fails, 'u' curvature test
// fails), each followed by an accepted trial.  gnorm0: |g| at the start (the first step is 1 / gnorm0).
static void drive(int ls, const std::vector<std::string>& searches, double gnorm0, bool positions) {
    bioen_lbfgs_config cfg{};
    cfg.linesearch = ls;
    cfg.max_iterations = 0;
    cfg.delta = 0.0;
    cfg.epsilon = 1e-30;
    cfg.ftol = 1e-4;
    cfg.gtol = 0.9;
    cfg.wolfe = 0.9;
    cfg.past = 0;
    cfg.max_linesearch = 100;
    LbfgsState m;
    lb::machine_reset(m, cfg, nullptr);
    double f = 1000.0;
    LbfgsAction act = lb::on_initial(m, cfg, f, gnorm0 * gnorm0, 1.0);
    CHECK(act.kind == ACT_TRIAL, "start: kind %d", act.kind);
    const double dginit = -1.0;
    for (size_t si = 0; si < searches.size() && act.kind != ACT_DONE; ++si) {
        const std::string& script = searches[si];
        std::vector<Issued> issued;
        int last = 0, prev = 0;
        for (size_t j = 0; j <= script.size(); ++j) {
            // before the trial: the generator's list, at full capacity and at every smaller one
            Issued is;
            is.last = last; is.prev = prev; is.iteration = m.iterations;
            is.n = lb::speculative_lattice(m.stp, ls, last, prev, m.iterations, lb::kLatticeMax, is.out);
            check_list(is.out, is.n, lb::kLatticeMax, "full list");
            for (int cap = 0; cap <= lb::kLatticeMax + 2; ++cap) {
                double part[lb::kLatticeMax + 2];
                const int np = lb::speculative_lattice(m.stp, ls, last, prev, m.iterations, cap, part);
                check_list(part, np, cap, "capped list");
                CHECK(np == (cap < is.n ? cap : is.n), "capacity %d gives %d of %d steps", cap, np, is.n);
                for (int i = 0; i < np && i < is.n; ++i) CHECK(same_bits(part[i], is.out[i]), "capacity %d changes step %d", cap, i);
            }
            issued.push_back(is);
            // the trial's made-up result
            const char mv = j < script.size() ? script[j] : 'a';
            TrialResult t{};
            t.dginit = dginit;
            t.gg = 1.0;
            t.xx = 1.0;
            const double armijo = m.ls.have_dginit ? m.ls.finit + m.stp * m.ls.dgtest : f + m.stp * cfg.ftol * dginit;
            if (mv == 'd') { t.f = armijo + 1.0; t.dg = 0.0; }
            else if (mv == 'u') { t.f = armijo - 1e-3; t.dg = 2.0 * dginit; }
            else if (mv == 'D') { t.f = armijo - 1e-3; t.dg = -10.0 * dginit; }
            else { t.f = armijo - 1e-3; t.dg = 0.0; }
            const double tried = m.stp;
            act = lb::on_trial(m, cfg, t);
            if (mv == 'a') {
                CHECK(act.kind == ACT_ACCEPT, "search %zu: accepting trial gives kind %d code %d", si, act.kind, act.code);
                f = t.f;
                break;
            }
            if (act.kind != ACT_TRIAL) break;       // the search ran out of its step bounds (the bounds scripts end so)
            const int dir = m.stp < tried ? -1 : +1;
            CHECK(dir == ((mv == 'u') ? +1 : -1), "search %zu move %zu: scripted %c, step went %+d", si, j, mv, dir);
            prev = last;
            last = dir;
            const bool inside = kMinStep <= m.stp && m.stp <= kMaxStep;
            for (Issued& e : issued) {
                e.moves.push_back(dir);
                const int idx = expected_index(ls, e.last, e.prev, e.iteration, e.moves);
                bool member = false;
                for (int i = 0; i < e.n; ++i) member = member || same_bits(e.out[i], m.stp);
                if (!inside) {
                    CHECK(!member, "a step outside the bounds (%g) is in a list", m.stp);
                } else if (positions && idx >= 0) {
                    CHECK(idx < e.n && same_bits(e.out[idx], m.stp),
                          "linesearch %d search %zu: after %zu moves the machine asks %.17g, the list has %.17g at %d (%d steps)", ls, si,
                          e.moves.size(), m.stp, idx < e.n ? e.out[idx] : 0.0, idx, e.n);
                } else if (idx >= 0 || e.moves.size() <= 2) {
                    CHECK(member, "linesearch %d search %zu: step %.17g after %zu moves is in no list", ls, si, m.stp, e.moves.size());
                }
            }
        }
    }
}

int main() {
    // linesearch 2 (Wolfe) and 3 (strong Wolfe): a first search with five "up", runs of "down", runs of "up", alternations
    const std::vector<std::string> wolfe = {"uuuuu", "ddd", "dddddd", "uuu", "uuuuuu", "dudu", "udud", "dududu", "", "d", "u",
                                            "dd", "uu", "du", "ud", "ddu", "uud", "ddud", "uudu", "ddddddd"};
    drive(2, wolfe, 1e3, true);
    drive(2, wolfe, 1.0, true);
    std::vector<std::string> strong = wolfe;
    for (const char* s : {"DDD", "DuDu", "uDuD", "dD", "Dd", "uD", "DDu"}) strong.push_back(s);
    drive(3, strong, 1e3, true);
    // a first search that goes down, and one that alternates
    drive(2, {"ddd", "uu"}, 1e-2, true);
    drive(2, {"udud", "dd"}, 1e-2, true);
    drive(3, {"DDDD"}, 1e-2, true);
    // linesearch 1 (Armijo): halvings only
    drive(1, {"ddddd", "", "d", "dddddddd", "dd"}, 1e3, true);
    drive(1, {"", "ddd"}, 1.0, true);
    // More-Thuente: nothing to foresee
    {
        double out[lb::kLatticeMax];
        CHECK(lb::speculative_lattice(1.0, 0, 0, 0, 3, lb::kLatticeMax, out) == 0, "More-Thuente gets candidates");
        CHECK(lb::speculative_lattice(1.0, 4, 0, 0, 3, lb::kLatticeMax, out) == 0, "an unknown line search gets candidates");
    }
    // at the step bounds: the first step is 1 / |g|; the searches walk out of [kMinStep, kMaxStep] and end there
    drive(2, {"uuuuuuuu"}, 1e-19, false);
    drive(2, {"dddddddd"}, 1e19, false);
    drive(3, {"DDDDDDDD"}, 0.5e20, false);
    drive(1, {"dddddddd"}, 1e19, false);
    drive(2, {"uuuuuuuu"}, 0.3e-19, false);
    std::printf("%ld checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}
