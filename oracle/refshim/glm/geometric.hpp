// Stand-in for <glm/geometric.hpp>: dot, cross, length, normalize, reflect, refract live in glm.hpp here.
#pragma once
#include "glm.hpp"
