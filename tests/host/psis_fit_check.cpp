// psis_fit_check — csrc/psis_fit.h alone on the host (tests/test_psis_fit_host.py builds it with the address and undefined-behaviour
// sanitizers and -ffp-contract=off).  Reads the file named by its argument, one case per line, numbers as C99 hex floats:
//   fit n t_0 ... t_{n-1}      -> "fit khat sigma q_0 q_mid q_last w_min_kept m_est": the fit of the ascending tail t, the smoothed
//                                 values (before truncation, with exp(cutoff) = 0) at ranks 0, n / 2 and n - 1, the smallest weight
//                                 at or above the 10 eps threshold
//   q p khat sigma             -> "q value": the quantile function
//   m S                        -> "m M": the tail length rule
// and ends with "psis_fit_check: ok <cases>".
#include "../../gpbayestools_hic_amd/csrc/psis_fit.h"

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

int main(int argc, char** argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: psis_fit_check <cases>\n");
        return 2;
    }
    std::ifstream in(argv[1]);
    if (!in) {
        std::fprintf(stderr, "psis_fit_check: cannot read %s\n", argv[1]);
        return 2;
    }
    std::string line;
    int cases = 0;
    while (std::getline(in, line)) {
        std::istringstream ss(line);
        std::string kind, tok;
        if (!(ss >> kind)) continue;
        std::vector<double> v;
        while (ss >> tok) v.push_back(std::strtod(tok.c_str(), nullptr));
        if (kind == "fit") {
            const int n = (int)v[0];
            if (n < GPB_PSIS_MIN_TAIL || n > GPB_PSIS_MAX_TAIL || (int)v.size() != n + 1) {
                std::fprintf(stderr, "psis_fit_check: bad fit case\n");
                return 1;
            }
            const int m = gpb::psis_m_est(n);
            std::vector<double> b(m), w(m);
            double khat, sigma;
            gpb::psis_fit_serial(v.data() + 1, n, &khat, &sigma, b.data(), w.data());
            double wmin = INFINITY;
            for (int i = 0; i < m; ++i)
                if (w[i] >= 10.0 * DBL_EPSILON && w[i] < wmin) wmin = w[i];
            std::printf("fit %a %a %a %a %a %a %d\n", khat, sigma, gpb::psis_smoothed(0, n, khat, sigma, 0.0),
                        gpb::psis_smoothed(n / 2, n, khat, sigma, 0.0), gpb::psis_smoothed(n - 1, n, khat, sigma, 0.0), wmin, m);
        } else if (kind == "q" && v.size() == 3) {
            std::printf("q %a\n", gpb::psis_gpd_quantile(v[0], v[1], v[2]));
        } else if (kind == "m" && v.size() == 1) {
            std::printf("m %lld\n", (long long)gpb::psis_tail_max((int64_t)v[0]));
        } else {
            std::fprintf(stderr, "psis_fit_check: bad line\n");
            return 1;
        }
        ++cases;
    }
    std::printf("psis_fit_check: ok %d\n", cases);
    return 0;
}
