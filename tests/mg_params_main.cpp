// Stand-alone driver of csrc/mg_params.cpp for tests/test_mg_params.py: one call per input line, one answer per output line.
//   input:   grid WHO ROWS NOTE nx ny nz smooth_steps over_correction min_rows      (NOTE: '-' = none, else '~' stands for a blank)
//            amg  WHO passes strength smooth_steps over_correction min_rows
//   output:  status nx ny nz smooth_steps min_rows omega algebraic passes theta | message
// *out is preset to a pattern no call produces, so an answer that leaves it alone shows.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

#include "../include/cgamd.h"
#include "mg_params.h"

static std::string g_message;
namespace cgamd {
int fail(int status, const std::string &msg) {
    g_message = msg;
    return status;
}
}  // namespace cgamd

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string kind, who, note, oc, strength;
        cgamd::MgParams p;
        p.nx = p.ny = p.nz = p.smooth_steps = p.min_rows = p.passes = -7;
        p.omega = p.theta = -7.;
        g_message.clear();
        int rc = -1;
        in >> kind >> who;
        if (kind == "grid") {
            long long rows;
            int nx, ny, nz, steps, min_rows;
            in >> rows >> note >> nx >> ny >> nz >> steps >> oc >> min_rows;
            for (char &c : note)
                if (c == '~') c = ' ';
            rc = cgamd::mg_params_grid(who, rows, note == "-" ? nullptr : note.c_str(), nx, ny, nz, steps, std::strtod(oc.c_str(), nullptr), min_rows, &p);
        } else if (kind == "amg") {
            int passes, steps, min_rows;
            in >> passes >> strength >> steps >> oc >> min_rows;
            rc = cgamd::mg_params_amg(who, passes, std::strtod(strength.c_str(), nullptr), steps, std::strtod(oc.c_str(), nullptr), min_rows, &p);
        }
        if (!in) {
            std::fprintf(stderr, "bad input line: %s\n", line.c_str());
            return 2;
        }
        std::printf("%d %d %d %d %d %d %.17g %d %d %.17g | %s\n", rc, p.nx, p.ny, p.nz, p.smooth_steps, p.min_rows, p.omega, p.algebraic ? 1 : 0,
                    p.passes, p.theta, g_message.c_str());
    }
    return 0;
}
