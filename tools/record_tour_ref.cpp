// record_tour_ref — runs the reference's own TSP::NearestNeighborSearch and TSP::TwoOptSearch
// (its include/TSPSolver.hpp, found on the include path given by tools/record_tour_ref.py) over one
// cost map read from stdin (V, then V * V ints) and prints "NN <path>" and "OPT <path>".  The
// reference's nearest-neighbour search prints each pick on a line of its own; the two marked lines
// are what the recorder reads.  A dead end aborts in the reference's assert: no marked line.
#include <climits>
#include <cstdio>
#include <iostream>

#include "TSPSolver.hpp"

int main() {
  int V = 0;
  if (!(std::cin >> V) || V < 0) return 2;
  std::vector<std::vector<int>> map(V, std::vector<int>(V));
  for (auto& row : map)
    for (int& e : row)
      if (!(std::cin >> e)) return 2;
  TSP::NearestNeighborSearch nn(map);
  nn.solve();
  std::vector<int> path = nn.getPath();
  std::cout << "NN";
  for (int x : path) std::cout << " " << x;
  std::cout << std::endl;
  TSP::TwoOptSearch opt(map);
  opt.setPath(path);
  opt.solve();
  std::cout << "OPT";
  for (int x : opt.getPath()) std::cout << " " << x;
  std::cout << std::endl;
  return 0;
}
