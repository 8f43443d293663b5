// Stand-alone load of .ski models through the host set-up (skirt_amd/csrc/host: build.cpp and the files it drives),
// no GPU and no Python: tools/ski_load_cpu.py builds it from those sources with the address and undefined-behaviour
// sanitizers, tests/test_ski_load.py runs it over tests/golden/ski/. Every model loads as the library loads it, on a
// Mersenne twister seeded from the model, worker threads included; one line per model: name, cells, sum of rho.
// Usage: ski_load_check <datadir> <model.ski> ...   (exit 1 when a model refuses to load)
#include <cstdio>
#include <exception>
#include <string>

#include "../skirt_amd/csrc/host/model.hpp"
#include "../skirt_amd/csrc/host/mt_random.hpp"
#include "../skirt_amd/csrc/host/outputs.hpp"

int main(int argc, char** argv) {
    if (argc < 3) {
        std::fprintf(stderr, "usage: %s <datadir> <model.ski> ...\n", argv[0]);
        return 2;
    }
    int refused = 0;
    for (int a = 2; a < argc; a++) {
        const std::string ski = argv[a];
        const std::string name = ski.substr(ski.rfind('/') + 1);
        try {
            skirt::MTRandom mt(skirt::readSkiSeed(ski));
            const skirt::Model m = skirt::loadSki(ski, mt, argv[1]);
            double sum = 0;
            for (double r : m.rho) sum += r;
            std::printf("%s %d %.17g\n", name.c_str(), m.ncells(), sum);
        } catch (std::exception& e) {
            std::printf("%s refused: %s\n", name.c_str(), e.what());
            refused++;
        }
    }
    return refused ? 1 : 0;
}
