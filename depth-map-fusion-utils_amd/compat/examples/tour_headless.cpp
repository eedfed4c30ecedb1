// tour_headless — the planners' run_tsp step through the drop-in header (compat/TSPSolver.hpp):
// a cost map from a text file (V, then V * V ints, row-major, whitespace-separated; INT_MAX = no
// edge), TSP::NearestNeighborSearch, then TSP::TwoOptSearch from its path.  Prints four lines: the
// nearest-neighbour path, its length (getPathLength(path): INT_MAX if an edge is INT_MAX), the
// 2-opt path and its length (tests/test_gpu_tour.py compares the paths with the recorded ones).
#include <cstdio>
#include <fstream>

#include "TSPSolver.hpp"

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: %s <cost map file>\n", argv[0]);
    return 2;
  }
  std::ifstream in(argv[1]);
  long long V = -1;
  if (!(in >> V) || V < 0 || V > 46340) {
    std::fprintf(stderr, "%s: no node count in 0..46340\n", argv[1]);
    return 2;
  }
  std::vector<std::vector<int>> map(V, std::vector<int>(V));
  for (auto& row : map)
    for (int& e : row)
      if (!(in >> e)) {
        std::fprintf(stderr, "%s: fewer than %lld entries\n", argv[1], V * V);
        return 2;
      }
  try {
    TSP::NearestNeighborSearch nn(map);
    nn.solve();
    std::vector<int> path = nn.getPath();
    nn.printPath();
    std::cout << nn.getPathLength(path) << std::endl;
    TSP::TwoOptSearch opt(map);
    opt.setPath(path);
    opt.solve();
    path = opt.getPath();
    opt.printPath();
    std::cout << opt.getPathLength(path) << std::endl;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "tour_headless: %s\n", e.what());
    return 1;
  }
  return 0;
}
